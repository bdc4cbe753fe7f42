// Stand-alone probe of csrc/onpolicy_plan.hpp (tests/test_onpolicy_plan.py compiles it with g++ -fsanitize=address,undefined — no hipcc,
// which is the proof that the header is free of HIP — and runs it): what an on-policy learn call decides before it touches the device.
// The expected values are written out here on their own: the arrays of each family in the order the kernels' argument structs have had
// since their ports, the scratch sizes as the entry points used to ask for them, the refusals' texts as the tests match them, the host
// shuffle's output as the loop of the commit before this header gave it.  Without arguments: every shape of the grid below, then
// "onpolicy_plan ok"; `perms T v0 v1 ..`: narrow_perms on these entries.  The first violated line and a non-zero exit otherwise.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "onpolicy_plan.hpp"

using namespace frl;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            printf("onpolicy_plan_probe.cpp:%d: %s\n", __LINE__, #cond);        \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

struct Span { size_t off, n; };
// disjoint, in this order, from 0, ending exactly at `total`
static void in_order(const std::vector<Span>& spans, size_t total) {
    size_t at = 0;
    for (const Span& s : spans) {
        CHECK(s.off == at);
        at += s.n;
    }
    CHECK(at == total);
}

static OnpolicyCall planned(OnpolicyFamily fam, size_t units, int T, int mb, int K, bool caller) {
    OnpolicyCall c;
    std::string why;
    const int rc = plan_onpolicy(fam, /*capacity*/ T, /*batch_max*/ mb, units, T, mb, K, caller, &c, &why);
    if (rc != FRL_OK) { printf("refused: %s\n", why.c_str()); exit(1); }
    return c;
}

static int shape(size_t P, size_t n, int T, int mb, int K) {
    const size_t U = P * n, n_mb = ((size_t)T + mb - 1) / mb;
    for (int fam = ONP_PPO; fam <= ONP_MAPPO; ++fam) {
        const size_t units = fam == ONP_MAPPO ? U : P;
        if (fam != ONP_MAPPO && n != 1) continue;      // (the single-agent families have no agent axis)
        const OnpolicyCall c = planned((OnpolicyFamily)fam, units, T, mb, K, false);
        CHECK(c.T == T && c.mb == mb && c.K == K && c.units == units && (size_t)c.n_mb == n_mb);
        CHECK(c.Tpad >= T && c.Tpad >= 2 && (c.Tpad & (c.Tpad - 1)) == 0 && (c.Tpad == 2 || c.Tpad / 2 < T));
        CHECK(c.perms == (T <= 8192 ? PERM_DEVICE : PERM_HOST));
        CHECK(planned((OnpolicyFamily)fam, units, T, mb, K, true).perms == PERM_CALLER);
        const size_t UT = units * T, trace = units * K * n_mb * 2;
        CHECK(c.rows() == UT && c.trace_n() == trace && c.perm_n() == units * K * T);
        if (fam == ONP_PPO) {
            const PpoLayout L = ppo_layout(c);
            in_order({{L.td, UT}, {L.vs, UT}, {L.adv_raw, UT}, {L.adv, UT}, {L.vtarget, UT}, {L.trace, trace}}, L.floats);
            CHECK(L.floats == P * ((size_t)5 * T + (size_t)K * n_mb * 2) && L.ints == P * (size_t)K * T);
        } else if (fam == ONP_GAIL_PPO) {
            const GailPpoLayout L = gail_ppo_layout(c);
            in_order({{L.vs, UT}, {L.logp_old, UT}, {L.td, UT}, {L.adv_raw, UT}, {L.adv, UT}, {L.returns, UT}, {L.rewards, UT}, {L.last_value, P},
                      {L.trace, trace}}, L.floats);
            CHECK(L.floats == 7 * UT + P + P * (size_t)K * n_mb * 2 && L.ints == P * (size_t)K * T);
        } else {
            for (int happo = 0; happo < 2; ++happo) {
                const MappoLayout L = mappo_layout(c, P, happo != 0);
                in_order({{L.td, UT}, {L.advd, UT}, {L.vs, UT}, {L.adv_seq, UT}, {L.adv_raw, UT}, {L.adv, UT}, {L.vtarget, UT}, {L.trace, trace},
                          {L.old, happo ? P * T : 0}, {L.factor, happo ? UT : 0}}, L.floats);
                in_order({{0, U * (size_t)K * T}, {L.order, happo ? U : 0}}, L.ints);
                CHECK(L.floats == 7 * U * T + trace + (happo ? (P + U) * T : 0) && L.ints == U * (size_t)K * T + (happo ? U : 0));
                CHECK(L.old == L.trace + trace && L.factor == L.old + (happo ? P * T : 0) && L.order == U * (size_t)K * T);
            }
        }
    }
    return 1;
}

static void refused(OnpolicyFamily fam, int capacity, int batch_max, int T, int mb, int K, const char* text, int line) {
    OnpolicyCall c;
    std::string why;
    const int rc = plan_onpolicy(fam, capacity, batch_max, 1, T, mb, K, false, &c, &why);
    if (rc != FRL_ERR_INVALID || why != text) { printf("onpolicy_plan_probe.cpp:%d: code %d \"%s\", expected \"%s\"\n", line, rc, why.c_str(), text); exit(1); }
}
#define REFUSED(fam, cap, bm, T, mb, K, text) refused(fam, cap, bm, T, mb, K, text, __LINE__)

static void refusals() {
    for (OnpolicyFamily fam : {ONP_PPO, ONP_MAPPO}) {
        REFUSED(fam, 40, 16, 1, 16, 1, "horizon 1 outside [2, capacity 40]");
        REFUSED(fam, 40, 16, 41, 16, 1, "horizon 41 outside [2, capacity 40]");
    }
    REFUSED(ONP_GAIL_PPO, 40, 16, 1, 16, 1, "horizon 1 < 2: the unbiased std of one advantage is NaN");
    REFUSED(ONP_GAIL_PPO, 40, 16, 41, 16, 1, "horizon 41 > capacity 40");
    for (OnpolicyFamily fam : {ONP_PPO, ONP_GAIL_PPO, ONP_MAPPO}) {
        REFUSED(fam, 40, 16, 40, 0, 1, "minibatch 0 outside [1,16]");
        REFUSED(fam, 40, 16, 40, 17, 1, "minibatch 17 outside [1,16]");
        REFUSED(fam, 40, 16, 40, 16, 0, "k_epochs must be >= 1");
        REFUSED(fam, 40, 16, 40, 16, -3, "k_epochs must be >= 1");
    }
}

static void shuffles() {
    // every block a permutation of 0..len-1, at the lengths of the grid's horizons and of HAPPO's visiting orders
    for (int len : {1, 2, 3, 40, 8192, 8193}) {
        std::vector<int> out;
        const size_t blocks = len > 100 ? 2 : 6;
        host_shuffle(20240607ull, 3, blocks, len, &out);
        CHECK(out.size() == blocks * (size_t)len);
        for (size_t b = 0; b < blocks; ++b) {
            std::vector<char> seen(len, 0);
            for (int i = 0; i < len; ++i) {
                const int v = out[b * len + i];
                CHECK(v >= 0 && v < len && !seen[v]);
                seen[v] = 1;
            }
        }
    }
    // the first block for two (seed, counter, len) triples, recorded from the entry points' own loop before it moved here
    std::vector<int> a, b;
    host_shuffle(20240607ull, 1, 2, 12, &a);
    host_shuffle(0x0123456789ABCDEFull, 7, 2, 5, &b);
    CHECK((std::vector<int>(a.begin(), a.begin() + 12) == std::vector<int>{1, 0, 9, 7, 4, 8, 6, 10, 5, 2, 11, 3}));
    CHECK((std::vector<int>(a.begin() + 12, a.end()) == std::vector<int>{8, 3, 4, 6, 0, 10, 7, 11, 9, 2, 5, 1}));      // (one stream over the blocks)
    CHECK((std::vector<int>(b.begin(), b.begin() + 5) == std::vector<int>{1, 3, 4, 2, 0}));
    CHECK((std::vector<int>(b.begin() + 5, b.end()) == std::vector<int>{3, 2, 0, 1, 4}));
}

int main(int argc, char** argv) {
    if (argc > 2 && !strcmp(argv[1], "perms")) {
        const int T = atoi(argv[2]);
        std::vector<int64_t> in;
        for (int i = 3; i < argc; ++i) in.push_back(atoll(argv[i]));
        std::vector<int> out;
        std::string why;
        if (narrow_perms(in.data(), in.size(), T, &out, &why) != FRL_OK) { printf("refused: %s\n", why.c_str()); return 1; }
        for (size_t i = 0; i < in.size(); ++i) CHECK(out[i] == (int)in[i]);
        printf("perms ok\n");
        return 0;
    }
    int shapes = 0;
    for (size_t P : {1, 3})
        for (size_t n : {1, 3})
            for (int T : {2, 40, 8192, 8193})
                for (int mb : {1, 16, T})
                    for (int K : {1, 3}) shapes += shape(P, n, T, mb, K);
    refusals();
    shuffles();
    printf("onpolicy_plan ok: %d shapes\n", shapes);
    return 0;
}
