"""Print per-kernel register / spill / scratch figures from hipcc's -save-temps assembly.
    FRL_HIP_VARIANT=dev FRL_HIPCC_FLAGS=-save-temps=obj python tools/kernel_regs.py [--check]"""
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FRL_HIP_VARIANT", "dev")
os.environ["FRL_HIPCC_FLAGS"] = os.environ.get("FRL_HIPCC_FLAGS", "") + " -save-temps=obj"
from freerl_amd import _native as N  # noqa: E402

if not (os.environ.get("FRL_REGS_REUSE") and os.path.exists(N.LIB_PATH)):
    N.build(force=True)
out_dir = os.path.dirname(N.LIB_PATH)                      # variants are built into tools/_bin/, next to their temporaries
asm = glob.glob(os.path.join(out_dir, "*gfx950.s"))[0]
s = open(asm).read()
md = s[s.index("amdhsa.kernels:"):]
# upper bounds on spilled VGPRs (`--check`: exit 1 when a kernel passes its bound — a regression gate for the hot kernels, which must
# stay spill-free, and a ratchet for the K-sliced / x-stationary / PPO ones, whose spills sit outside their MFMA loops: DESIGN.md 8)
# (round 6: the lane constants re-derived per phase took the K-sliced kernels from 97-397 spilled VGPRs to 0-51, PPO's from 135-140 to 0)
BOUNDS = [("ac_critic_v2_", 8), ("ac_actor_v2_", 0), ("solo_critic_twin_w8_", 8), ("solo_", 0), ("solow_", 0), ("dqn_fused_", 0), ("c51_grad_", 0), ("ac_critic_kernel", 0),
          ("ac_critic_wide_", 60), ("ac_actor_wide_", 16), ("ac_critic_x_", 700), ("ac_actor_x_", 460), ("ppo_update_v2_", 0),
          ("sacd_critic_", 9), ("sacd_actor_", 0),
          # kernels_reinforce.hip: reinforce_returns_kernel 48 VGPRs, reinforce_grad_kernel 248 VGPRs; no spilled VGPR in either (the grad
          # kernel keeps 56 bytes of its row lambda's captures in scratch: stored at entry, three loads per row chunk, none in an MFMA loop)
          ("reinforce_returns_", 0), ("reinforce_grad_", 0),
          # kernels_envelope.hip: envelope_weights_kernel 38 VGPRs, none spilled; envelope_grad_kernel 256 VGPRs with 8 spilled and 88 bytes of
          # scratch (the Lds carve and the chunk loop's bounds, as in sacd_critic_kernel: reloaded per pass or per row chunk, none in an MFMA loop)
          ("envelope_weights_", 0), ("envelope_grad_", 8),
          # kernels_envelope_ddpg.hip: both kernels 256 VGPRs; the actor 18 spilled and 128 bytes of scratch, the critic 15 and 116 (two NetDescs' layer offsets, the Lds carve
          # and the chunk loop's bounds: stored at entry, reloaded per pass or per row chunk, none in an MFMA loop)
          ("envelope_ddpg_critic_", 18), ("envelope_ddpg_actor_", 18),
          # kernels_gail.hip: gail_disc_kernel 256 VGPRs with 69 spilled and 288 bytes of scratch: values that live across the whole chunk loop
          # (the per-row partial sums, the layers' offsets, the Lds carve, the row counts) are stored at entry (55 of the 62 scratch stores) and
          # reloaded at the start of a barrier phase or between two tile blocks of a dW phase (tools/asm_spills.py), none inside an MFMA k-loop;
          # gail_forward_kernel 188 VGPRs, gail_draw_kernel 28, gail_stats_kernel 19, none spilled
          # kernels_gail_ppo.hip (the unit compiled on its own, profiles/gail_ppo/README.md): gail_ppo_update_kernel 300 VGPRs + 48 AGPRs (one
          # persistent workgroup per net, one wave per SIMD), gail_ppo_prepare_kernel 192 + 40, gail_ppo_act_kernel 188 + 40, gail_ppo_gae_kernel 16;
          # no spilled VGPR in any, 56 bytes of scratch in the three forward kernels (a lambda's captures, as in reinforce_grad_kernel)
          ("gail_ppo_", 0),
          ("gail_disc_", 70), ("gail_forward_", 0), ("gail_draw_", 0), ("gail_stats_", 0),
          # kernels_mappo.hip: mappo_update_kernel 375 VGPRs + 119 AGPRs (one persistent workgroup per CU: one wave per SIMD, 512 registers),
          # mappo_values_kernel 224 + 40, mappo_act_kernel 188 + 40, mappo_adv_kernel 17; no spilled VGPR in any, 56 bytes of scratch in the three
          # forward kernels (a lambda's captures, as in reinforce_grad_kernel: none in an MFMA loop)
          ("mappo_update_", 0), ("mappo_values_", 0), ("mappo_act_", 0), ("mappo_adv_", 0),
          # kernels_happo.hip: happo_update_kernel = mappo_update_kernel's steps (device/mappo.hpp: mappo_steps) between two forward-only
          # horizon passes, one persistent workgroup per CU as well: 355 VGPRs + 99 AGPRs, no spilled VGPR, 56 bytes of scratch (with the step
          # loop shared, mappo_update_kernel keeps its 375 + 119 and holds 72 bytes of scratch, the lambda's captures again)
          ("happo_", 0),
          # kernels_mappo_mask.hip: mappo_mask_update_kernel = mappo_steps with the masked categorical row in its discrete branch, 369 VGPRs +
          # 113 AGPRs and 72 bytes of scratch; mappo_mask_act_kernel = mappo_act_kernel's forward with the masked draw behind it, 188 + 40 and
          # 56 bytes; no spilled VGPR in either (mappo_update_kernel and happo_update_kernel keep their figures)
          ("mappo_mask_", 0),
          # kernels_mappo_state.hip: mappo_steps with the critic's row filled from two segments (kState): mappo_state_update_kernel and
          # mappo_state_mask_update_kernel 370 VGPRs + 114 AGPRs and 72 bytes of scratch, mappo_state_values_kernel = mappo_values_kernel's
          # 224 + 40 and 56 bytes; no spilled VGPR in any of the three (the other kernels of the family keep their figures)
          ("mappo_state_", 0),
          # kernels_att.hip (figures of the unit compiled on its own, profiles/att/README.md): the attention critic's forward and backward are
          # two non-inlined device functions (device/att.hpp), so their ~25 linear_* call sites' lane addresses live inside them instead of
          # at the kernels' top: att_critic_kernel 256 VGPRs + 44 AGPRs, no spilled VGPR, 96 bytes of scratch (the Lds / AttLds structs the
          # calls pass by reference); att_q_kernel the same, none spilled; att_actor_kernel 77 spilled and 368 bytes: the actor's own inlined
          # mlp_fwd_rows / mlp_bwd addresses, stored at entry and reloaded at the start of a barrier phase, none inside an MFMA k-loop
          ("att_critic_", 0), ("att_actor_", 77), ("att_q_", 0),
          # kernels_masac.hip (figures of the unit compiled on its own, DESIGN.md "MASAC"): masac_critic_kernel 256 VGPRs, no spilled VGPR, 56 bytes of
          # scratch (a row lambda's captures); masac_act_kernel 188 VGPRs + 40 AGPRs, none spilled; masac_actor_kernel 256 VGPRs with 49 spilled and
          # 220 bytes: the two NetDescs' layer offsets, the three draw-set bases and the chunk loop's bounds, stored at entry and reloaded at the
          # start of a barrier phase or between two tile blocks, none inside an innermost MFMA k-loop (some outer layer / tile-block loops hold them)
          ("masac_critic_", 0), ("masac_actor_", 52), ("masac_act_", 0),
          # kernels_her.hip (the unit compiled on its own): her_relabel_kernel 29 VGPRs, 60 SGPRs, no spilled VGPR, no scratch (byte work)
          ("her_", 0),
          # kernels_cem_gd3pg.hip (the unit compiled on its own, profiles/cem_gd3pg/kernel_regs.txt): cem_critic_kernel 256 VGPRs with 44 spilled and
          # 204 bytes of scratch — seven forward passes and a backward over three nets' layer offsets, the Lds carve, the chunk loop's bounds and two
          # per-row sums: stored at entry, reloaded at the start of a pass, none of its 102 scratch accesses inside an innermost MFMA k-loop;
          # cem_actor_kernel 255 VGPRs, none spilled, 56 bytes (a row lambda's captures); cem_act_kernel 188 + 40 AGPRs; cem_draw_kernel 106; cem_step_kernel 61
          ("cem_critic_", 44), ("cem_actor_", 0), ("cem_", 0), ("", 20)]
bad = []
for blk in md.split("  - .agpr_count:")[1:]:
    g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
    short = re.sub(r"^_ZN3frl\d+", "", g("name"))
    bound = next(b for pre, b in BOUNDS if short.startswith(pre))
    if int(g("vgpr_spill_count")) > bound:
        bad.append("%s: %s spilled VGPRs > %d" % (short[:40], g("vgpr_spill_count"), bound))
    print("%-34s agpr %3s vgpr %3s spill %3s scratch %4s" % (re.sub(r"^_ZN3frl\d+", "", g("name"))[:34], blk.split()[0],
          g("vgpr_count"), g("vgpr_spill_count"), g("private_segment_fixed_size")))
for f in glob.glob(os.path.join(out_dir, "frl_api-*")) + glob.glob(os.path.join(out_dir, "frl_api.hip-*")) + [N.LIB_PATH]:      # leave nothing for gpurun to ship
    if os.environ.get("FRL_KEEP_ASM") and f.endswith(".s"):
        continue
    os.remove(f)
if "--check" in sys.argv:
    if bad:
        print("spill bounds exceeded:\n  " + "\n  ".join(bad))
        sys.exit(1)
    print("spill bounds hold")
