// The grouping of the twin search (control_amd/csrc/spectrum_host.hpp: group_twins, twin_classes)
// on forged fingerprints, in plain C++.
//
// A candidate is (shift bits, folded fingerprint, value id); two candidates have equal bits when
// their value ids are equal.  The "device" comparison of a pair is the comparison of the ids, so a
// forged fingerprint can say "equal" where the bits differ -- the collision no real build reaches.
// Checked per case: every pair is (first of the group, a later member) of one (shift, fingerprint);
// the number of pairs is the number of candidates minus the number of groups; two candidates share
// a class only when shift and values are equal; a candidate whose comparison failed has no class
// and nobody shares with it; classes are numbered in the order of their first members.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "spectrum_host.hpp"

namespace spec = kkt::spec;

struct Cand {
    uint64_t shift, fp;
    int values;
};

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("%s: ", name);                       \
            std::printf(__VA_ARGS__);                        \
            std::printf("  [%s]\n", #cond);                  \
            ++failures;                                      \
        }                                                    \
    } while (0)

// runs the grouping; want_cls: the expected class per candidate (-1: none)
static void run(const char *name, const std::vector<Cand> &c, const std::vector<int> &want_cls) {
    const int C = (int)c.size();
    std::vector<uint64_t> shifts(C), fps(C);
    for (int i = 0; i < C; ++i) shifts[i] = c[i].shift, fps[i] = c[i].fp;
    spec::TwinGroups T = spec::group_twins(shifts, fps);
    std::set<std::pair<uint64_t, uint64_t>> groups;
    for (int i = 0; i < C; ++i) groups.insert({shifts[i], fps[i]});
    CHECK((int)T.pairs.size() == C - (int)groups.size(), "%zu pairs, %d candidates, %zu groups",
          T.pairs.size(), C, groups.size());
    CHECK((int)T.first_of.size() == C && (int)T.pair_of.size() == C, "sizes");
    for (int i = 0; i < C; ++i) {
        const int f = T.first_of[i];
        CHECK(f >= 0 && f <= i, "first_of[%d] = %d", i, f);
        CHECK(shifts[f] == shifts[i] && fps[f] == fps[i], "candidate %d grouped across keys", i);
        CHECK(T.first_of[f] == f, "the first of %d is not a first", i);
        for (int j = 0; j < f; ++j)
            CHECK(!(shifts[j] == shifts[i] && fps[j] == fps[i]), "%d is not the first of %d", f, i);
        if (f == i) {
            CHECK(T.pair_of[i] == -1, "a first with a pair");
        } else {
            CHECK(T.pair_of[i] >= 0 && T.pair_of[i] < (int)T.pairs.size(), "pair_of[%d]", i);
            if (T.pair_of[i] >= 0 && T.pair_of[i] < (int)T.pairs.size())
                CHECK(T.pairs[T.pair_of[i]] == std::make_pair(f, i), "pair of %d", i);
        }
    }
    std::vector<unsigned> differ;
    for (const auto &p : T.pairs) differ.push_back(c[p.first].values != c[p.second].values);
    std::vector<int> reps;
    const std::vector<int> cls = spec::twin_classes(T, differ, &reps);
    CHECK(cls == want_cls, "classes differ from the expected ones");
    for (int i = 0; i < C; ++i) {
        std::printf("%s  candidate %d: shift %llu fingerprint %llu values %d -> class %d (expected %d)\n", name,
                    i, (unsigned long long)c[i].shift, (unsigned long long)c[i].fp, c[i].values,
                    i < (int)cls.size() ? cls[i] : -99, want_cls[i]);
        for (int j = 0; j < i && i < (int)cls.size(); ++j)
            if (cls[i] >= 0 && cls[i] == cls[j])
                CHECK(c[i].shift == c[j].shift && c[i].values == c[j].values, "a false twin: %d and %d", j, i);
    }
    // classes in order of their first members
    int next = 0;
    for (int i = 0; i < C && i < (int)cls.size(); ++i)
        if (cls[i] == next) {
            CHECK(next < (int)reps.size() && reps[next] == i, "rep of class %d", next);
            ++next;
        } else {
            CHECK(cls[i] < next, "class numbers are not in creation order at %d", i);
        }
    CHECK(next == (int)reps.size(), "%d classes, %zu reps", next, reps.size());
}

int main() {
    // no twins: every candidate its own class, no pair
    run("no twins", {{1, 10, 0}, {1, 11, 1}, {2, 12, 2}, {2, 13, 3}}, {0, 1, 2, 3});
    // all twins: one class, C - 1 pairs against the first
    run("all twins", {{7, 5, 0}, {7, 5, 0}, {7, 5, 0}, {7, 5, 0}, {7, 5, 0}}, {0, 0, 0, 0, 0});
    // equal fingerprints (and equal values) under different shifts: never paired
    run("shifts", {{1, 5, 0}, {2, 5, 0}, {1, 5, 0}, {3, 5, 0}, {2, 5, 0}}, {0, 1, 0, 2, 1});
    // a collision: A, then B with A's fingerprint but other bits, then C equal to B.  B and C are
    // both compared with A, the group's first: neither gets a class, neither shares with A.
    run("collision", {{1, 5, 0}, {1, 5, 1}, {1, 5, 1}}, {0, -1, -1});
    // the same among true twins and other groups
    run("collision among twins",
        {{1, 5, 0}, {1, 6, 2}, {1, 5, 1}, {1, 5, 0}, {1, 6, 2}, {4, 5, 1}, {1, 5, 1}, {4, 5, 1}},
        {0, 1, -1, 0, 1, 2, -1, 2});
    // one candidate, and none
    run("one", {{1, 5, 0}}, {0});
    run("none", {}, {});
    std::printf("twin groups: %d failures\n", failures);
    return failures ? 1 : 0;
}
