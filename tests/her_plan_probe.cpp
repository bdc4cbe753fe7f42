// csrc/her_plan.h on the CPU (g++ -std=c++17 -fsanitize=address,undefined, tests/test_her_plan.py): every (capacity, cursor, L,
// sample_num, sample_range) of a small grid is either refused for the rule this file works out on its own, or walked — the prefix
// offsets are a bijection onto [0, total), her_locate inverts them, every source and destination row is inside the ring, and no
// destination row is a source row.
//   her_plan_probe            the walk; prints "her_plan ok <accepted> <refused>"
//   her_plan_probe --totals   "L k R total" per line, for the Python side to compare with its own formula
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "her_plan.h"

using namespace frl;

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                    \
            std::fprintf(stderr, "\n");                           \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

static long long brute_total(int L, int k, int R) {
    long long t = 0;
    for (int i = 0; i < L; ++i) {
        int n = k < R ? k : R;
        if (L - i < n) n = L - i;
        t += n;
    }
    return t;
}

static const int kCaps[] = {8, 13, 64}, kKs[] = {1, 2, 4, 8}, kRs[] = {1, 2, 5, 200};

static void walk(int capacity, int cursor, int L, int k, int R) {
    const HerPlan p = her_plan(capacity, cursor, L, k, R);
    const long long total = her_total(p);
    CHECK(total == brute_total(L, k, R), "total %lld at L %d k %d R %d", total, L, k, R);
    std::vector<char> is_src((size_t)capacity, 0), is_dst((size_t)capacity, 0), hit((size_t)total, 0);
    const int start = her_start(p);
    CHECK(start >= 0 && start < capacity && (start + L) % capacity == cursor, "start %d", start);
    for (int i = 0; i < L; ++i) {
        const int row = her_src(p, i);
        CHECK(row >= 0 && row < capacity, "src(%d) = %d", i, row);
        CHECK(row == (start + i) % capacity, "src(%d) = %d", i, row);
        CHECK(!is_src[row], "source row %d twice", row);
        is_src[row] = 1;
        const int m = her_m(p, i), n = her_n(p, i);
        CHECK(m == (R < L - i ? R : L - i) && n == (k < m ? k : m) && n >= 1, "m %d n %d at i %d", m, n, i);
        CHECK(i + m <= L, "candidates of %d past the episode", i);      // every pick i + o, o < m, is a source row of the episode
        for (int s = 0; s < n; ++s) {
            const long long r = her_prefix(p, i) + s;
            CHECK(r >= 0 && r < total && !hit[(size_t)r], "ordinal %lld of (%d, %d)", r, i, s);
            hit[(size_t)r] = 1;
            int i2 = -1, s2 = -1;
            her_locate(p, r, i2, s2);
            CHECK(i2 == i && s2 == s, "locate(%lld) = (%d, %d), not (%d, %d)", r, i2, s2, i, s);
        }
    }
    for (long long r = 0; r < total; ++r) {
        CHECK(hit[(size_t)r], "ordinal %lld unused", r);
        const int row = her_dst(p, r);
        CHECK(row >= 0 && row < capacity && row == (int)((cursor + r) % capacity), "dst(%lld) = %d", r, row);
        CHECK(!is_dst[row], "destination row %d twice", row);
        CHECK(!is_src[row], "destination row %d is a source row", row);
        is_dst[row] = 1;
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--totals") {
        for (int L : {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 40, 200})
            for (int k : kKs)
                for (int R : kRs) std::printf("%d %d %d %lld\n", L, k, R, her_total(her_plan(1 << 20, 0, L, k, R)));
        return 0;
    }
    long long accepted = 0, refused = 0;
    const HerShape good{6, 3, 3, 4, 200};
    for (int capacity : kCaps)
        for (int L = 0; L <= 12; ++L)
            for (int k : kKs)
                for (int R : kRs) {
                    HerShape s = good;
                    s.sample_num = k; s.sample_range = R;
                    for (int size : {0, L - 1, L, capacity}) {
                        if (size < 0 || size > capacity) continue;
                        const HerRefusal want = L < 1 ? HER_EMPTY_EPISODE : L > size ? HER_EPISODE_NOT_STORED
                                              : L + brute_total(L, k, R) > capacity ? HER_NO_ROOM : HER_OK;
                        const HerRefusal got = her_check(s, capacity, size, L);
                        CHECK(got == want, "capacity %d size %d L %d k %d R %d: %s, expected %s", capacity, size, L, k, R, her_refusal_text(got), her_refusal_text(want));
                        if (got != HER_OK) { ++refused; continue; }
                        for (int cursor = 0; cursor < capacity; ++cursor) { walk(capacity, cursor, L, k, R); ++accepted; }
                    }
                }
    CHECK(accepted > 1000 && refused > 1000, "%lld accepted, %lld refused", accepted, refused);
    // the shape rules, each named before any episode rule, in the order of the header
    struct Bad { HerShape s; HerRefusal want; };
    const Bad bad[] = {
        {{6, 3, 3, 0, 200}, HER_BAD_SAMPLE_NUM}, {{6, 3, 3, 9, 200}, HER_BAD_SAMPLE_NUM}, {{6, 3, 3, -1, 0}, HER_BAD_SAMPLE_NUM},
        {{6, 3, 3, 4, 0}, HER_BAD_SAMPLE_RANGE}, {{6, 3, 3, 8, -5}, HER_BAD_SAMPLE_RANGE},
        {{6, 3, 0, 4, 200}, HER_BAD_GOAL_DIM}, {{7, 3, 4, 4, 200}, HER_BAD_GOAL_DIM}, {{6, 0, 0, 4, 200}, HER_BAD_GOAL_DIM}, {{6, 3, -1, 4, 200}, HER_BAD_GOAL_DIM},
        {{7, 3, 3, 4, 200}, HER_BAD_OBS_DIM}, {{6, 5, 2, 4, 200}, HER_BAD_OBS_DIM}, {{5, 3, 3, 4, 200}, HER_BAD_OBS_DIM},
    };
    for (const Bad& b : bad)
        for (int L : {0, 1, 100}) {          // ... whatever the episode is
            const HerRefusal got = her_check(b.s, 8, 4, L);
            CHECK(got == b.want, "shape (%d %d %d %d %d): %s, expected %s", b.s.obs_dim, b.s.state_dim, b.s.goal_dim, b.s.sample_num, b.s.sample_range,
                  her_refusal_text(got), her_refusal_text(b.want));
            ++refused;
        }
    CHECK(her_check({7, 5, 2, 8, 1}, 64, 64, 12) == HER_OK, "S 5 G 2");
    // ring arithmetic at the largest ring an int cursor can index
    const HerPlan big = her_plan(0x7fffffff, 5, 200, 4, 200);
    CHECK(her_start(big) == 0x7fffffff - 195 && her_src(big, 199) == 4 && her_dst(big, 793) == 798 && her_total(big) == 794, "large ring");
    std::printf("her_plan ok %lld %lld\n", accepted, refused);
    return 0;
}
