// Stand-alone probe of the CEM_GD3PG engine's plan and addressing (csrc/engine_plan.hpp, csrc/rowchunk_layout.h): tests/test_cem_gd3pg_plan.py
// compiles it with g++ -fsanitize=address,undefined (no hipcc) and runs it on a file of shapes, one per line
//     <name> <obs_dim> <act_dim> <hidden> <n_learners> <capacity> <batch_max> <rc knob> <cps knob> <rows> [<rows> ...]
// For every shape and call size it decodes every block id of the critic launch (units = learners) and of the actor launch (units =
// (learner, actor)) the way learner_unit / cem_actor_unit do, walks the workgroup's chunks, and checks every offset that
// kernels_cem_gd3pg.hip forms — idx, the parked domain rows, part slots, slabs, spill blocks, ring rows, the step kernel's blocks, the
// LDS carve — against what the plan allocates, and that no two workgroups own the same slab region, part float or spill block.
// One line per shape, or the first violated assertion with its numbers and a non-zero exit.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "engine_plan.hpp"

using namespace frl;

#define WALK_CHECK(cond, ...)                                                                      \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            printf("%s: rows %d: %s violated:", name.c_str(), rows, #cond);                        \
            printf(" " __VA_ARGS__);                                                               \
            printf("\n");                                                                          \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

struct Region { size_t off, n; };
static bool disjoint(std::vector<Region> v, size_t* a, size_t* b) {
    std::sort(v.begin(), v.end(), [](const Region& x, const Region& y) { return x.off < y.off; });
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i - 1].off + v[i - 1].n > v[i].off) { *a = v[i - 1].off; *b = v[i].off; return false; }
    return true;
}

// learner_unit's decoding of a block id (csrc/device/update_common.hpp): -> (unit, slice)
static void decode(int block, int ns, int* unit, int* sl) {
    const int group = 8 * ns, g = block / group, l = block - g * group;
    *unit = g * 8 + (l & 7);
    *sl = l >> 3;
}

static void walk(const std::string& line) {
    std::istringstream in(line);
    std::string name;
    int O, A, H, P, cap, bm, rc_knob, cps_knob;
    in >> name >> O >> A >> H >> P >> cap >> bm >> rc_knob >> cps_knob;
    std::vector<int> sizes;
    for (int r; in >> r;) sizes.push_back(r);
    int rows = 0;
    WALK_CHECK(!sizes.empty(), "no call sizes");
    frl_config c;
    memset(&c, 0, sizeof c);
    c.algo = FRL_ALGO_CEM_GD3PG; c.n_learners = P; c.n_agents = 1; c.obs_dim[0] = O; c.act_dim[0] = A;
    c.hidden = H; c.hidden_act = FRL_ACT_TANH; c.capacity = cap; c.batch_max = bm;
    PlanKnobs knobs;
    knobs.rc = rc_knob; knobs.cps = cps_knob;
    EnginePlan pl;
    std::string why;
    const int prc = plan_engine(c, nullptr, PlanLimits(), knobs, &pl, &why);
    WALK_CHECK(prc == FRL_OK, "refused: %s", why.c_str());
    const EngineDesc& h = pl.h;
    // the plan itself: four nets, two rings side by side, the carve
    WALK_CHECK(h.n_nets == 4 && pl.n_rings == 2 && pl.ring_cap == cap && h.capacity == 2 * cap, "nets %d rings %d cap %d / %d", h.n_nets, pl.n_rings, pl.ring_cap, h.capacity);
    WALK_CHECK(h.net[0].hidden_act == ACT_TANH && h.net[1].hidden_act == ACT_TANH && h.net[3].hidden_act == ACT_TANH && h.net[2].hidden_act == ACT_LEAKY_RELU, "activations");
    WALK_CHECK(h.net[0].size == h.net[1].size && h.net[0].size == h.net[3].size, "actor sizes");
    if (rc_knob) WALK_CHECK(h.rc == rc_knob, "rc %d", h.rc);
    WALK_CHECK(pl.lds_bytes == lds_bytes_for(h, h.rc) && pl.lds_bytes <= 160 * 1024, "lds %d", pl.lds_bytes);
    const int kc0 = h.net[2].L[0].k_pad, ka0 = h.net[0].L[0].k_pad;
    WALK_CHECK(h.lds_kin_pad >= kc0 && kc0 >= ka0 && kc0 >= O + A && ka0 >= O, "xin %d holds [obs | act] %d", h.lds_kin_pad, kc0);
    WALK_CHECK(h.lds_act_pad >= A && h.act_max == A && h.lds_batch_pad >= h.rc && h.lds_hbufs == 2, "abuf %d act_max %d y %d", h.lds_act_pad, h.act_max, h.lds_batch_pad);
    WALK_CHECK(h.lds_out_pad >= h.net[0].L[2].n_pad && h.lds_out_pad >= h.net[2].L[2].n_pad, "outb %d", h.lds_out_pad);
    WALK_CHECK(h.rec.act_off[0] == h.rec.obs_off[0] + O && h.rec.width <= h.rec.stride, "record");
    WALK_CHECK(pl.act_spill_count == cem_spill_floats(h) && h.noise_sets >= 1, "spill count");
    const size_t replay_floats = (size_t)P * h.capacity * h.rec.stride, param_floats = (size_t)P * h.learner_stride;
    long long walked = 0;
    for (int r : sizes) {
        rows = r;
        WALK_CHECK(rows >= 2 && rows % 2 == 0 && rows <= h.batch_max, "batch_max %d", h.batch_max);
        const int n_chunks = rowchunk_chunks(h, rows), ns = rowchunk_ns(h, rows);
        WALK_CHECK(ns >= 1 && ns <= h.S, "ns %d S %d", ns, h.S);
        for (int launch = 0; launch < 2; ++launch) {      // 0: cem_critic_kernel, 1: cem_actor_kernel
            const int units = launch == 0 ? P : kCemActors * P, grid = ((units + 7) / 8) * 8 * ns;
            std::vector<Region> slabs, parts, spills;
            std::map<std::pair<int, int>, int> seen;          // (unit, slice) -> workgroups
            std::map<int, int> next;                          // unit -> rows covered by its slices so far
            for (int b = 0; b < grid; ++b) {
                int unit, sl;
                decode(b, ns, &unit, &sl);
                WALK_CHECK(sl >= 0 && sl < ns, "block %d slice %d of %d", b, sl, ns);
                if (unit >= units) continue;                  // the 8-aligned grid's spare workgroups return at once
                const int p = launch == 0 ? unit : unit / kCemActors, actor = launch == 0 ? -1 : unit % kCemActors;
                WALK_CHECK(p >= 0 && p < P, "block %d learner %d", b, p);
                const int times = ++seen[std::make_pair(unit, sl)];
                WALK_CHECK(times == 1, "block %d: (unit %d, slice %d) twice", b, unit, sl);
                const ChunkRange cr = chunk_range(h, rows, sl);
                WALK_CHECK(cr.c0 < cr.c1 && cr.c1 <= n_chunks, "slice %d chunks [%d, %d) of %d", sl, cr.c0, cr.c1, n_chunks);
                for (int ck = cr.c0; ck < cr.c1; ++ck, ++walked) {
                    const RowChunk ch = row_chunk(cr, ck);
                    WALK_CHECK(ch.nv >= 1 && ch.nv <= h.rc && ch.r0 + ch.nv <= rows, "chunk %d rows [%d, %d)", ck, ch.r0, ch.r0 + ch.nv);
                    WALK_CHECK(ch.gs == (ck == cr.c0 ? (h.cps > 1 ? GS_STORE : GS_STREAM) : GS_ADD), "chunk %d gs %d", ck, ch.gs);
                    next[unit] += ch.nv;
                    WALK_CHECK(idx_offset(h, p, 0, ch.r0) + ch.nv <= pl.idx_count, "idx %zu + %d > %zu", idx_offset(h, p, 0, ch.r0), ch.nv, pl.idx_count);
                    // the parked domain rows: inside set 0 of the learner's noise block, pitch act_max
                    const size_t d0 = cem_domain_offset(h, p, ch.r0), dn = (size_t)ch.nv * h.act_max;
                    WALK_CHECK(d0 + dn <= pl.noise_count && d0 >= noise_offset(h, p, 0, 0, 0) && d0 + dn <= noise_offset(h, p, 0, 0, 0) + noise_set_floats(h),
                               "domain rows %zu + %zu outside set 0 at %zu (+ %zu) of %zu", d0, dn, noise_offset(h, p, 0, 0, 0), noise_set_floats(h), pl.noise_count);
                    // a batch row reads a record of either ring: the largest absolute row is h.capacity - 1
                    WALK_CHECK(((size_t)p * h.capacity + (h.capacity - 1)) * h.rec.stride + h.rec.width <= replay_floats, "ring row of learner %d", p);
                }
                // what the workgroup owns: the critic launch its slice's critic slab and part floats {0, 1}; actor j its net's slab, part float 2 + j, a spill block
                const int net = launch == 0 ? 2 : actor;
                WALK_CHECK(slab_offset(h, p, sl, net) + h.net[net].size <= pl.slab_count, "slab of net %d: %zu + %d > %zu", net, slab_offset(h, p, sl, net), h.net[net].size, pl.slab_count);
                slabs.push_back({slab_offset(h, p, sl, net), (size_t)h.net[net].size});
                WALK_CHECK(part_offset(h, p, 0, sl) + kPartFloats <= pl.part_count, "part %zu + 4 > %zu", part_offset(h, p, 0, sl), pl.part_count);
                if (launch == 0) parts.push_back({part_offset(h, p, 0, sl) + CEM_PART_CRITIC, 2});
                else parts.push_back({part_offset(h, p, 0, sl) + CEM_PART_ACTOR + actor, 1});
                if (launch == 1) {
                    WALK_CHECK(cem_spill_offset(h, p, actor, sl) + act_spill_pitch(h) <= pl.act_spill_count, "spill %zu + %d > %zu", cem_spill_offset(h, p, actor, sl),
                               act_spill_pitch(h), pl.act_spill_count);
                    spills.push_back({cem_spill_offset(h, p, actor, sl), (size_t)act_spill_pitch(h)});
                    // cem_c2_sum reads the slices' part slots 0 .. ns-1 of the learner
                    WALK_CHECK(part_offset(h, p, 0, 0) + (size_t)kPartFloats * ns <= pl.part_count, "c2 slots of learner %d", p);
                }
            }
            WALK_CHECK((int)seen.size() == units * ns, "%zu workgroups for %d units x %d slices", seen.size(), units, ns);
            for (const auto& kv : next) WALK_CHECK(kv.second == rows, "unit %d covers %d rows", kv.first, kv.second);
            size_t a = 0, b = 0;
            WALK_CHECK(disjoint(slabs, &a, &b), "launch %d: slab regions at %zu and %zu", launch, a, b);
            WALK_CHECK(disjoint(parts, &a, &b), "launch %d: part floats at %zu and %zu", launch, a, b);
            WALK_CHECK(disjoint(spills, &a, &b), "launch %d: spill blocks at %zu and %zu", launch, a, b);
        }
        // cem_step_kernel: a trained net's blocks of grad / theta / m / v / target, its slices' slabs, the learner's counters and outputs
        for (int p = 0; p < P; ++p)
            for (int net = 0; net < 3; ++net) {
                WALK_CHECK((size_t)p * h.learner_stride + h.net_off[net] + h.net[net].size <= param_floats && h.net[net].size % 4 == 0, "net %d of learner %d", net, p);
                WALK_CHECK(slab_offset(h, p, ns - 1, net) + h.net[net].size <= pl.slab_count, "last slab of net %d", net);
                WALK_CHECK((size_t)p * (kMaxNets + 1) + net < pl.steps_count, "step counter");
            }
        // cem_draw_kernel: both halves of a learner's idx row
        WALK_CHECK(idx_offset(h, P - 1, 0, 0) + rows <= pl.idx_count, "idx of the last learner");
    }
    printf("%s: rc %d cps %d S %d lds %d: %lld chunks walked\n", name.c_str(), h.rc, h.cps, h.S, pl.lds_bytes, walked);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: cem_gd3pg_plan_probe <shapes file>\n"); return 2; }
    std::ifstream f(argv[1]);
    if (!f.good()) { printf("cannot read %s\n", argv[1]); return 2; }
    for (std::string line; std::getline(f, line);)
        if (!line.empty()) walk(line);
    return 0;
}
