// Stand-alone probe of csrc/engine_plan.hpp (tests/test_engine_plan.py compiles it with g++ -fsanitize=address,undefined — no hipcc,
// which is the proof that the header is free of HIP — and runs it).  Without arguments: the create-time literals the GPU suite states,
// "engine_plan ok" or a message and a non-zero exit.  With a file of configurations, one per line
//     <name> <frl_config bytes, hex> <frl_config_ext bytes, hex | -> <n_cus> <lds_per_cu> [<PlanKnobs field>=<int>]...
// one JSON object per line: what describe() of tests/test_gpu_algo_matrix.py reads off an engine, or {refused, message}.
// With --walk and such a file: every (unit, slice, chunk) of the row-chunk launch shape (csrc/rowchunk_layout.h) at each configuration's
// call sizes, against the plan's buffer counts — one line per configuration, or the first violated assertion with its numbers.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "engine_plan.hpp"

using namespace frl;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            printf("engine_plan_probe.cpp:%d: %s\n", __LINE__, #cond);         \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static LearnPath path_of(const EnginePlan& pl, int batch) {      // frl_learn_path with no per-call knob set
    const LearnFamily fam = learn_family(pl.h, pl.family, batch, true);
    return learn_path(pl.h, pl, fam, batch, dqn_split_for(pl.h, batch, pl.h.P, -1));
}

// ---------------------------------------------------------------------------------- literals
static frl_config config(int algo, std::vector<int> obs, std::vector<int> act, int hidden, int batch_max, int n_learners = 1, bool twin = false) {
    frl_config c;
    memset(&c, 0, sizeof c);
    c.algo = algo;
    c.n_learners = n_learners;
    c.n_agents = (int)obs.size();
    for (size_t j = 0; j < obs.size(); ++j) { c.obs_dim[j] = obs[j]; c.act_dim[j] = act[j]; }
    c.discrete = algo == FRL_ALGO_DQN;
    c.hidden = hidden;
    c.hidden_act = FRL_ACT_RELU;
    c.twin_critic = twin;
    c.capacity = 512;
    c.batch_max = batch_max;
    return c;
}

static EnginePlan planned(const frl_config& c, const PlanKnobs& knobs = PlanKnobs()) {
    EnginePlan pl;
    std::string why;
    const int rc = plan_engine(c, nullptr, PlanLimits(), knobs, &pl, &why);
    if (rc != FRL_OK) { printf("refused: %s\n", why.c_str()); exit(1); }
    return pl;
}

static void literals() {
    // tests/test_gpu_config_shapes.py: the one-launch DQN update at a batch of 256
    LearnPath p = path_of(planned(config(FRL_ALGO_DQN, {8}, {4}, 128, 256)), 256);
    CHECK(p.chained && p.bytes == 77184 && p.rows == 64);
    // ... kernels_solow.hip (160 512 B of LDS, a 16-row tile per workgroup) while every workgroup of a launch fits the chip
    struct Case { frl_config c; int batch; bool solow; };
    const std::vector<int> O3{18, 18, 18}, A3{5, 5, 5};
    const Case cases[] = {
        {config(FRL_ALGO_SAC, {376}, {17}, 128, 256, 1, true), 256, true},
        {config(FRL_ALGO_TD3, {17}, {6}, 128, 256, 16, true), 256, true},
        {config(FRL_ALGO_TD3, {17}, {6}, 128, 256, 17, true), 256, false},
        {config(FRL_ALGO_DDPG, {8}, {6}, 128, 100), 100, true},                    // act > 4: past the narrow kernels
        {config(FRL_ALGO_MADDPG, O3, A3, 128, 1024), 1024, true},                  // 3 x 64 workgroups
        {config(FRL_ALGO_MADDPG, O3, A3, 128, 1024, 2), 1024, false},              // 6 x 64 do not fit
        {config(FRL_ALGO_MADDPG, O3, A3, 128, 128, 5), 128, true},                 // 15 units x 16
        {config(FRL_ALGO_MADDPG, O3, A3, 128, 128, 6), 128, false},
        {config(FRL_ALGO_SAC, {376}, {17}, 256, 256, 1, true), 256, false},
    };
    for (const Case& k : cases) {
        p = path_of(planned(k.c), k.batch);
        if (k.solow) CHECK(p.chained && p.bytes == 160512 && p.rows == 16);
        else CHECK(!p.chained);
    }
    // tests/test_gpu_algo_matrix.py, sac/wide_input: Humanoid's 393 critic columns at hidden 256, 16 rows bumped to 32
    frl_config wide = config(FRL_ALGO_SAC, {376}, {17}, 256, 32, 1, true);
    wide.capacity = 40;
    const EnginePlan pw = planned(wide);
    CHECK(pw.h.rc == 32 && pw.lds_bytes > 80 * 1024);
    // a plan carries no device pointer
    CHECK(!pw.h.theta && !pw.h.replay && !pw.h.slab && !pw.h.obsnorm && !pw.h.wide_scr);
    // a refusal leaves its text and builds nothing that needs undoing; an unusable configuration cannot overrun the descriptor
    frl_config bad = config(FRL_ALGO_TD3, {8}, {2}, 128, 256);
    bad.n_agents = 100;
    EnginePlan pb;
    std::string why;
    CHECK(plan_engine(bad, nullptr, PlanLimits(), PlanKnobs(), &pb, &why) == FRL_ERR_INVALID && why == "n_agents out of range");
}

// ---------------------------------------------------------------------------- the matrix
static bool unhex(const std::string& s, void* out, size_t n) {
    if (s.size() != 2 * n) return false;
    for (size_t i = 0; i < n; ++i) ((unsigned char*)out)[i] = (unsigned char)std::stoi(s.substr(2 * i, 2), nullptr, 16);
    return true;
}

static std::string json_string(const std::string& s) {
    std::string o = "\"";
    for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; }
    return o + "\"";
}

template <class T>
static std::string json_list(const T* v, int n) {
    std::string o = "[";
    for (int i = 0; i < n; ++i) o += (i ? ", " : "") + std::to_string(v[i]);
    return o + "]";
}

static std::string json_path(const EnginePlan& pl, int batch) {
    if (algo_traits(pl.h.algo).learn != kFrlLearn) return "null";      // (describe(): the kinds frl_learn updates)
    const LearnPath p = path_of(pl, batch);
    return std::string("[") + (p.chained ? "true" : "false") + ", " + std::to_string(p.bytes) + ", " + std::to_string(p.rows) + "]";
}

static void set_knob(PlanKnobs& k, const std::string& name, int v) {
    if (name == "assume_cus") k.assume_cus = v;
    else if (name == "rc") k.rc = v;
    else if (name == "cps") k.cps = v;
    else if (name == "solow_narrow") k.solow_narrow = v != 0;
    else if (name == "critic_v2") k.critic_v2 = v;
    else if (name == "solo") k.solo = v;
    else if (name == "solo_maxp") k.solo_maxp = v;
    else if (name == "solow") k.solow = v;
    else if (name == "solow_helpers") k.solow_helpers = v != 0;
    else if (name == "chain_waves") k.chain_waves = v;
    else { printf("unknown knob %s\n", name.c_str()); exit(1); }
}

// a line of the configuration file -> (name, plan or refusal)
struct Planned { std::string name, why; int rc; EnginePlan pl; };
static Planned plan_line(const std::string& line) {
    std::istringstream in(line);
    std::string cfg_hex, ext_hex, tok;
    Planned out;
    PlanLimits limits;
    in >> out.name >> cfg_hex >> ext_hex >> limits.n_cus >> limits.lds_per_cu;
    frl_config c;
    frl_config_ext x;
    CHECK(in && unhex(cfg_hex, &c, sizeof c) && (ext_hex == "-" || unhex(ext_hex, &x, sizeof x)));
    PlanKnobs knobs;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        CHECK(eq != std::string::npos);
        set_knob(knobs, tok.substr(0, eq), atoi(tok.c_str() + eq + 1));
    }
    out.rc = plan_engine(c, ext_hex == "-" ? nullptr : &x, limits, knobs, &out.pl, &out.why);
    return out;
}

static void describe(const std::string& line) {
    const Planned P = plan_line(line);
    const std::string &name = P.name, &why = P.why;
    const EnginePlan& pl = P.pl;
    const int rc = P.rc;
    std::cout << "{\"name\": " << json_string(name);
    if (rc != FRL_OK) {
        std::cout << ", \"refused\": " << rc << ", \"message\": " << json_string(why) << "}\n";
        return;
    }
    const EngineDesc& h = pl.h;
    int n_params[kMaxNets];
    for (int i = 0; i < h.n_nets; ++i) n_params[i] = h.net[i].n_params;
    frl_record_layout lay;
    record_layout(h.rec, &lay);
    std::cout << ", \"lds_bytes\": " << pl.lds_bytes << ", \"row_chunk\": " << h.rc << ", \"n_nets\": " << h.n_nets
              << ", \"n_params\": " << json_list(n_params, h.n_nets) << ", \"layout\": {\"n_agents\": " << lay.n_agents << ", \"width\": " << lay.width
              << ", \"stride\": " << lay.stride << ", \"obs_off\": " << json_list(lay.obs_off, FRL_MAX_AGENTS) << ", \"obs_dim\": "
              << json_list(lay.obs_dim, FRL_MAX_AGENTS) << ", \"act_off\": " << json_list(lay.act_off, FRL_MAX_AGENTS) << ", \"act_dim\": "
              << json_list(lay.act_dim, FRL_MAX_AGENTS) << ", \"rew_off\": " << lay.rew_off << ", \"done_off\": " << lay.done_off
              << ", \"next_obs_off\": " << json_list(lay.next_obs_off, FRL_MAX_AGENTS) << ", \"extra_off\": " << lay.extra_off
              << ", \"extra\": " << lay.extra << "}, \"learn_path\": " << json_path(pl, 8) << ", \"learn_path_max\": " << json_path(pl, h.batch_max) << "}\n";
}

// ---------------------------------------------------------------------------------- the walk
#define WALK_CHECK(cond, ...)                                                                      \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            printf("%s: rows %d: %s violated:", name.c_str(), rows, #cond);                        \
            printf(" " __VA_ARGS__);                                                               \
            printf("\n");                                                                          \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

// [off, off + n) regions of one buffer, each owned by one (unit, slice): sorted, none may reach into the next
struct Region { size_t off, n; };
static bool disjoint(std::vector<Region> v, size_t* a, size_t* b) {
    std::sort(v.begin(), v.end(), [](const Region& x, const Region& y) { return x.off < y.off; });
    for (size_t i = 1; i < v.size(); ++i)
        if (v[i - 1].off + v[i - 1].n > v[i].off) { *a = v[i - 1].off; *b = v[i].off; return false; }
    return true;
}

static void walk(const std::string& line) {
    const Planned P = plan_line(line);
    const std::string& name = P.name;
    if (P.rc != FRL_OK) { printf("%s: refused\n", name.c_str()); return; }
    const EnginePlan& pl = P.pl;
    const EngineDesc& h = pl.h;
    if (!pl.has_nets) { printf("%s: no nets\n", name.c_str()); return; }
    // the rows one call may bring (the entry points' own limits): GAIL n_expert + n_policy of 1 .. batch_max each, REINFORCE an episode
    // of 2 .. capacity (= batch_max) steps, the envelope engines batch x weight_num <= batch_max, every other engine batch <= batch_max
    const bool gail = h.algo == ALGO_GAIL;
    const int min_rows = gail || h.algo == ALGO_REINFORCE ? 2 : 1, max_rows = gail ? 2 * h.batch_max : h.batch_max;
    const int sizes[] = {1, h.rc - 1, h.rc, h.rc + 1, max_rows};
    long long walked = 0;
    for (int rows : sizes) {
        if (rows < min_rows || rows > max_rows) continue;
        const int n_chunks = rowchunk_chunks(h, rows), ns = rowchunk_ns(h, rows);
        WALK_CHECK(ns >= 1 && ns <= h.S, "ns %d S %d", ns, h.S);
        std::vector<Region> slabs, parts, spills;
        for (int p = 0; p < h.P; ++p)
            for (int ag = 0; ag < h.n_agents; ++ag) {
                int next = 0;      // the chunk the next slice must start at
                for (int sl = 0; sl < ns; ++sl) {
                    WALK_CHECK(sl < h.S, "sl %d S %d", sl, h.S);
                    const ChunkRange cr = chunk_range(h, rows, sl, gail);
                    WALK_CHECK(cr.c0 == next && cr.c1 > cr.c0 && cr.c1 <= n_chunks, "sl %d range [%d, %d) after %d of %d", sl, cr.c0, cr.c1, next, n_chunks);
                    next = cr.c1;
                    for (int ck = cr.c0; ck < cr.c1; ++ck, ++walked) {
                        const RowChunk c = row_chunk(cr, ck);
                        WALK_CHECK(c.nv >= 1 && c.r0 + c.nv <= rows, "chunk %d rows [%d, %d)", ck, c.r0, c.r0 + c.nv);
                        WALK_CHECK(c.first == (ck == cr.c0) && c.gs == (c.first ? ((h.cps > 1 || gail) ? GS_STORE : GS_STREAM) : GS_ADD), "chunk %d gs %d", ck, c.gs);
                        if (c.r0 + c.nv > h.batch_max) continue;      // (GAIL's policy rows: staged rows, no idx entry and no draw)
                        WALK_CHECK(idx_offset(h, p, ag, c.r0) + c.nv <= pl.idx_count, "idx %zu + %d > %zu", idx_offset(h, p, ag, c.r0), c.nv, pl.idx_count);
                        for (int set = 0; set < h.noise_sets; ++set)
                            WALK_CHECK(noise_offset(h, p, ag, set, c.r0) + (size_t)c.nv * h.act_max <= pl.noise_count, "noise set %d: %zu + %d x %d > %zu", set,
                                       noise_offset(h, p, ag, set, c.r0), c.nv, h.act_max, pl.noise_count);
                    }
                    for (int i = 0; i < h.n_nets; ++i) {
                        WALK_CHECK(h.net_off[i] + h.net[i].size <= h.learner_stride, "net %d: %d + %d > stride %d", i, h.net_off[i], h.net[i].size, h.learner_stride);
                        WALK_CHECK(slab_offset(h, p, sl, i) - h.net_off[i] + h.learner_stride <= pl.slab_count, "slab of net %d: %zu > %zu", i,
                                   slab_offset(h, p, sl, i) - h.net_off[i] + h.learner_stride, pl.slab_count);
                        if (ag == 0) slabs.push_back({slab_offset(h, p, sl, i), (size_t)h.net[i].size});      // (one slab per (learner, slice): the agents' nets side by side)
                    }
                    WALK_CHECK(part_offset(h, p, ag, sl) + kPartFloats <= pl.part_count, "part %zu + 4 > %zu", part_offset(h, p, ag, sl), pl.part_count);
                    parts.push_back({part_offset(h, p, ag, sl), (size_t)kPartFloats});
                    if (pl.act_spill_count) {
                        WALK_CHECK(act_spill_offset(h, p, ag, sl) + act_spill_pitch(h) <= pl.act_spill_count, "act_spill %zu + %d > %zu", act_spill_offset(h, p, ag, sl),
                                   act_spill_pitch(h), pl.act_spill_count);
                        spills.push_back({act_spill_offset(h, p, ag, sl), (size_t)act_spill_pitch(h)});
                    }
                }
                WALK_CHECK(next == n_chunks, "the slices end at chunk %d of %d", next, n_chunks);
            }
        size_t a = 0, b = 0;
        WALK_CHECK(disjoint(slabs, &a, &b), "slab regions at %zu and %zu", a, b);
        WALK_CHECK(disjoint(parts, &a, &b), "part slots at %zu and %zu", a, b);
        WALK_CHECK(disjoint(spills, &a, &b), "act_spill blocks at %zu and %zu", a, b);
    }
    printf("%s: rc %d cps %d S %d: %lld chunks walked\n", name.c_str(), h.rc, h.cps, h.S, walked);
}

int main(int argc, char** argv) {
    literals();
    if (argc < 2) { printf("engine_plan ok\n"); return 0; }
    const bool walking = std::string(argv[1]) == "--walk";
    CHECK(argc > (walking ? 2 : 1));
    std::ifstream f(argv[walking ? 2 : 1]);
    CHECK(f.good());
    for (std::string line; std::getline(f, line);)
        if (!line.empty()) walking ? walk(line) : describe(line);
    return 0;
}
