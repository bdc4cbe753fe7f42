// Stand-alone probe of csrc/actor_park_layout.h and of what csrc/engine_plan.hpp plans for it (tests/test_actor_park_layout.py compiles
// it with g++ -fsanitize=address,undefined — no hipcc — and runs it).
//     actor_park_probe walk <learners>     every (learner, chunk, tile, wave, lane) slot: "slots <n> max_end_bytes <b> overlaps <k>"
//     actor_park_probe plan <file>         lines as tests/engine_plan_probe.cpp reads them -> "<name>: family <f> floats <n>" or "<name>: refused"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "engine_plan.hpp"

using namespace frl;

static bool unhex(const std::string& s, void* out, size_t n) {
    if (s.size() != 2 * n) return false;
    for (size_t i = 0; i < n; ++i) ((unsigned char*)out)[i] = (unsigned char)std::stoi(s.substr(2 * i, 2), nullptr, 16);
    return true;
}

static int walk(int P) {
    const size_t slot_bytes = kParkSlotFloats * sizeof(float);
    const size_t n = (size_t)P * kParkChunks * kParkTiles * kParkWaves * kParkLanes;
    std::vector<unsigned char> seen(n + 1, 0);      // (+1: a slot one past the end is counted, not written out of bounds)
    size_t max_end = 0, overlaps = 0, outside = 0;
    for (int p = 0; p < P; ++p)
        for (int c = 0; c < kParkChunks; ++c)
            for (int t = 0; t < kParkTiles; ++t)
                for (int w = 0; w < kParkWaves; ++w)
                    for (int l = 0; l < kParkLanes; ++l) {
                        const size_t s = actor_park_slot(p, c, t, w, l);
                        if (s >= n) { ++outside; continue; }
                        overlaps += seen[s];
                        seen[s] = 1;
                        if ((s + 1) * slot_bytes > max_end) max_end = (s + 1) * slot_bytes;
                    }
    // a wave instruction (fixed learner, chunk, tile, wave) covers 1 KB contiguously: lane l at the wave's base + 16 l bytes
    size_t ragged = 0;
    for (int l = 0; l < kParkLanes; ++l) ragged += actor_park_slot(P - 1, kParkChunks - 1, kParkTiles - 1, kParkWaves - 1, l) != actor_park_slot(P - 1, kParkChunks - 1, kParkTiles - 1, kParkWaves - 1, 0) + l;
    // the same lane's consecutive tiles lie kParkTileStride slots apart (what the kernel steps by)
    ragged += actor_park_slot(0, 0, 1, 0, 0) - actor_park_slot(0, 0, 0, 0, 0) != (size_t)kParkTileStride;
    printf("slots %zu max_end_bytes %zu planned_bytes %zu overlaps %zu outside %zu ragged %zu\n", n, max_end, actor_park_floats(P) * sizeof(float), overlaps, outside,
           ragged);
    return 0;
}

static int plan(const char* path) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string name, cfg_hex, ext_hex, tok;
        PlanLimits limits;
        in >> name >> cfg_hex >> ext_hex >> limits.n_cus >> limits.lds_per_cu;
        frl_config c;
        frl_config_ext x;
        if (!in || !unhex(cfg_hex, &c, sizeof c) || !(ext_hex == "-" || unhex(ext_hex, &x, sizeof x))) { printf("%s: bad line\n", name.c_str()); return 1; }
        PlanKnobs knobs;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            const std::string k = tok.substr(0, eq);
            const int v = atoi(tok.c_str() + eq + 1);
            if (k == "assume_cus") knobs.assume_cus = v;
            else if (k == "rc") knobs.rc = v;
            else if (k == "cps") knobs.cps = v;
            else if (k == "solow_narrow") knobs.solow_narrow = v != 0;
            else if (k == "critic_v2") knobs.critic_v2 = v;
            else if (k == "solo") knobs.solo = v;
            else if (k == "solo_maxp") knobs.solo_maxp = v;
            else if (k == "solow") knobs.solow = v;
            else if (k == "solow_helpers") knobs.solow_helpers = v != 0;
            else if (k == "chain_waves") knobs.chain_waves = v;
            else if (k == "actor_park") knobs.actor_park = v != 0;
            else { printf("unknown knob %s\n", k.c_str()); return 1; }
        }
        EnginePlan pl;
        std::string why;
        if (plan_engine(c, ext_hex == "-" ? nullptr : &x, limits, knobs, &pl, &why) != FRL_OK) { printf("%s: refused\n", name.c_str()); continue; }
        printf("%s: family %d floats %zu park %d null %d\n", name.c_str(), (int)pl.family, pl.actor_park_count, (int)pl.actor_park, pl.h.actor_park == nullptr);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "walk") return walk(atoi(argv[2]));
    if (argc == 3 && std::string(argv[1]) == "plan") return plan(argv[2]);
    printf("usage: actor_park_probe walk <learners> | plan <file>\n");
    return 2;
}
