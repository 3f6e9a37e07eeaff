// The run partition of the preconditioner program (control_amd/csrc/program_partition.hpp:
// partition_program, what SchurPC::fuse_programs cuts its steps with) on hand-written step lists,
// in plain C++.  Each case names its steps, the four switches, what the tile form answers, where the
// data-flow chain breaks, and the pieces and tile candidates it expects, in order.
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "program_partition.hpp"

using kkt::Piece;
using kkt::StepDesc;

static int failures = 0;

// a single-block ROWS step outside the levels; of level `lv`; a COARSE step of level `lv`
static StepDesc rows() { return StepDesc{StepDesc::ROWS, true, -1, false}; }
static StepDesc of_level(int lv, bool eligible) { return StepDesc{StepDesc::ROWS, true, lv, eligible}; }
static StepDesc coarse(int lv, bool eligible) { return StepDesc{StepDesc::COARSE, true, lv, eligible}; }
// what ends a run: a ROWS step with several ops, a TIME or COMM step
static StepDesc multi() { return StepDesc{StepDesc::ROWS, false, -1, false}; }
static StepDesc other() { return StepDesc{StepDesc::OTHER, false, -1, false}; }

static std::vector<StepDesc> repeat(int n, StepDesc d) { return std::vector<StepDesc>((size_t)n, d); }
static std::vector<StepDesc> operator+(std::vector<StepDesc> a, const std::vector<StepDesc> &b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
// `count` levels of `steps` steps each, numbered from `from`, all eligible but `bad`
static std::vector<StepDesc> levels(int count, int steps, int from = 0, int bad = -1) {
    std::vector<StepDesc> d;
    for (int l = 0; l < count; ++l) d = d + repeat(steps, of_level(from + l, from + l != bad));
    return d;
}

struct Switches {
    bool use_tiles, sharded, legacy_ok, prog_granule;
};
using Range = std::pair<size_t, size_t>;

static const char *kind_name(Piece::Kind k) {
    return k == Piece::KEEP ? "keep" : k == Piece::PLAIN ? "plain" : k == Piece::PROGRAM ? "program" : "tiles";
}

static void run(const char *name, const std::vector<StepDesc> &d, Switches sw, bool tiles_answer,
                const std::set<size_t> &chain_breaks, const std::vector<Piece> &want,
                const std::vector<Range> &want_asked) {
    std::vector<Range> asked;
    const std::vector<Piece> got = kkt::partition_program(
        d, sw.use_tiles, sw.sharded, sw.legacy_ok, sw.prog_granule,
        [&](size_t a, size_t b) {
            asked.push_back({a, b});
            return tiles_answer;
        },
        [&](size_t q) { return chain_breaks.count(q) == 0; });
    bool same = got.size() == want.size() && asked == want_asked;
    for (size_t i = 0; same && i < got.size(); ++i)
        same = got[i].kind == want[i].kind && got[i].first == want[i].first && got[i].last == want[i].last;
    // whatever the case: the pieces tile the step list in order
    size_t at = 0;
    bool tiling = true;
    for (const Piece &p : got) {
        tiling = tiling && p.first == at && p.last > p.first;
        at = p.last;
    }
    tiling = tiling && at == d.size();
    std::printf("%-34s", name);
    for (const Piece &p : got) std::printf(" %s[%zu,%zu)", kind_name(p.kind), p.first, p.last);
    std::printf("  asked");
    for (const Range &r : asked) std::printf(" [%zu,%zu)", r.first, r.second);
    std::printf("%s%s\n", same ? "" : "  DIFFERENT from the expected list", tiling ? "" : "  DIFFERENT: not a tiling");
    if (!same || !tiling) ++failures;
}

int main() {
    const Switches tiles{true, false, true, false}, shard{true, true, true, false};
    const Switches flow{true, false, true, true};      // data-flow programs: chains() is asked
    const Piece::Kind KEEP = Piece::KEEP, PLAIN = Piece::PLAIN, PROGRAM = Piece::PROGRAM, TILES = Piece::TILES;

    run("three steps stay plain", repeat(3, rows()), tiles, true, {}, {{PLAIN, 0, 3}}, {});
    run("four steps are a program", repeat(4, rows()), tiles, true, {}, {{PROGRAM, 0, 4}}, {});
    run("four steps, no row programs", repeat(4, rows()), {true, false, false, false}, true, {},
        {{PLAIN, 0, 4}}, {});
    run("six levels, tiles take them", levels(6, 4), tiles, true, {}, {{TILES, 0, 24}}, {{0, 24}});
    run("six levels, tiles refuse", levels(6, 4), flow, false, {4, 8, 12, 16, 20},
        {{PROGRAM, 0, 4}, {PROGRAM, 4, 8}, {PROGRAM, 8, 12}, {PROGRAM, 12, 16}, {PROGRAM, 16, 20},
         {PROGRAM, 20, 24}},
        {{0, 24}});
    run("six levels, tiles not wanted", levels(6, 4), {false, false, true, false}, true, {},
        {{PROGRAM, 0, 24}}, {});
    // the whole run goes to the rest path: the tile form is not asked
    run("an ineligible level in the middle", levels(5, 4, 0, 2), tiles, true, {}, {{PROGRAM, 0, 20}}, {});
    {
        // two two-grid levels: update, correction, two sweeps each
        std::vector<StepDesc> d;
        for (int l = 0; l < 2; ++l)
            d = d + repeat(1, of_level(l, true)) + repeat(1, coarse(l, true)) + repeat(2, of_level(l, true));
        run("a COARSE step, tiles refuse", d, tiles, false, {}, {{PLAIN, 0, 8}}, {{0, 8}});
        run("a COARSE step, tiles take", d, tiles, true, {}, {{TILES, 0, 8}}, {{0, 8}});
    }
    run("chain breaks after step 5 of 9", repeat(9, rows()), flow, true, {5},
        {{PROGRAM, 0, 5}, {PROGRAM, 5, 9}}, {});
    run("chain breaks after step 2 of 9", repeat(9, rows()), flow, true, {2},
        {{PLAIN, 0, 2}, {PROGRAM, 2, 9}}, {});
    run("breaks are not asked (counters)", repeat(9, rows()), tiles, true, {2, 5}, {{PROGRAM, 0, 9}}, {});
    {
        // a one-level time shard: products, the level, a product in one run
        const std::vector<StepDesc> d = repeat(2, rows()) + levels(1, 6) + repeat(1, rows());
        run("one-level shard", d, shard, true, {}, {{PLAIN, 0, 2}, {TILES, 2, 8}, {PLAIN, 8, 9}}, {{2, 8}});
        run("one-level shard, tiles refuse", d, shard, false, {}, {{PROGRAM, 0, 9}}, {{2, 8}});
        run("the same run on one rank", d, tiles, true, {}, {{PROGRAM, 0, 9}}, {});
    }
    run("one-level shard, a short level", levels(1, 3), shard, true, {}, {{PLAIN, 0, 3}}, {});
    {
        // two stretches of levels with products between them and four in front
        const std::vector<StepDesc> d =
            repeat(4, rows()) + levels(2, 4) + repeat(1, rows()) + levels(1, 5, 2) + repeat(1, rows());
        run("shard, two stretches", d, shard, true, {},
            {{PROGRAM, 0, 4}, {TILES, 4, 12}, {PLAIN, 12, 13}, {TILES, 13, 18}, {PLAIN, 18, 19}},
            {{4, 12}, {13, 18}});
    }
    {
        const std::vector<StepDesc> d = repeat(4, rows()) + repeat(1, multi()) + repeat(4, rows()) +
                                        repeat(1, other()) + repeat(4, rows()) + repeat(2, other()) +
                                        repeat(1, rows());
        run("multi-op ROWS, TIME, COMM end a run", d, tiles, true, {},
            {{PROGRAM, 0, 4}, {KEEP, 4, 5}, {PROGRAM, 5, 9}, {KEEP, 9, 10}, {PROGRAM, 10, 14}, {KEEP, 14, 16},
             {PLAIN, 16, 17}},
            {});
    }
    run("no steps", {}, tiles, true, {}, {}, {});
    std::printf("program partition: %d failures\n", failures);
    return failures ? 1 : 0;
}
