// Stand-alone probe of csrc/engine_plan.hpp (tests/test_engine_plan.py compiles it with g++ -fsanitize=address,undefined — no hipcc,
// which is the proof that the header is free of HIP — and runs it).  Without arguments: the create-time literals the GPU suite states,
// "engine_plan ok" or a message and a non-zero exit.  With a file of configurations, one per line
//     <name> <frl_config bytes, hex> <frl_config_ext bytes, hex | -> <n_cus> <lds_per_cu> [<PlanKnobs field>=<int>]...
// one JSON object per line: what describe() of tests/test_gpu_algo_matrix.py reads off an engine, or {refused, message}.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

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

static void describe(const std::string& line) {
    std::istringstream in(line);
    std::string name, cfg_hex, ext_hex, tok;
    PlanLimits limits;
    in >> name >> cfg_hex >> ext_hex >> limits.n_cus >> limits.lds_per_cu;
    frl_config c;
    frl_config_ext x;
    CHECK(in && unhex(cfg_hex, &c, sizeof c) && (ext_hex == "-" || unhex(ext_hex, &x, sizeof x)));
    PlanKnobs knobs;
    while (in >> tok) {
        const size_t eq = tok.find('=');
        CHECK(eq != std::string::npos);
        set_knob(knobs, tok.substr(0, eq), atoi(tok.c_str() + eq + 1));
    }
    EnginePlan pl;
    std::string why;
    const int rc = plan_engine(c, ext_hex == "-" ? nullptr : &x, limits, knobs, &pl, &why);
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

int main(int argc, char** argv) {
    literals();
    if (argc < 2) { printf("engine_plan ok\n"); return 0; }
    std::ifstream f(argv[1]);
    CHECK(f.good());
    for (std::string line; std::getline(f, line);)
        if (!line.empty()) describe(line);
    return 0;
}
