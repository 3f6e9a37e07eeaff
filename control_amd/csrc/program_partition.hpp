// How SchurPC::fuse_programs (pc_lower.cpp) cuts the emitted steps into pieces: which stay as
// they are, which become one tile launch sequence, which a row program.  Only the control flow:
// what a step is comes in as a StepDesc, what the tile form and the data-flow program accept as
// two predicates.  Host-only, nothing here knows HIP (tests/native/program_partition.cpp).
#pragma once
#include <cstddef>
#include <vector>

namespace kkt {

struct StepDesc {
    enum Kind { ROWS, COARSE, OTHER } kind = OTHER;
    bool single = false;     // a single-block step: a ROWS step with one op, or a COARSE step
    int level = -1;          // the sweep level it belongs to
    bool eligible = false;   // ... which the tile form can express
};

struct Piece {
    // KEEP: steps outside the runs of single-block steps; PLAIN: single-block steps that stay plain
    // launches; PROGRAM: one row program; TILES: whole sweep levels the tile form took
    enum Kind { KEEP, PLAIN, PROGRAM, TILES } kind;
    size_t first, last;      // steps [first, last)
};

// Every maximal run of single-block steps: tile launches if it has >= 4 steps, is exactly a run of
// eligible levels and tiles_take(a, b) accepts it; on a time shard every stretch of >= 4 steps of
// eligible levels inside it that tiles_take accepts; what is left ("the rest") stays plain where
// it holds a COARSE step, else it is cut where chains(q) -- step q gathers exactly what step q - 1
// produced, asked for the data-flow form only -- breaks, and parts of >= 4 steps become row programs.
// tiles_take is called once per candidate, in step order, and a candidate it took is a piece.
template <class TilesTake, class Chains>
std::vector<Piece> partition_program(const std::vector<StepDesc> &d, bool use_tiles, bool sharded,
                                     bool legacy_ok, bool prog_granule, TilesTake tiles_take,
                                     Chains chains) {
    std::vector<Piece> out;
    auto push = [&](Piece::Kind kind, size_t a, size_t b) {
        if ((kind == Piece::KEEP || kind == Piece::PLAIN) && !out.empty() && out.back().kind == kind &&
            out.back().last == a)
            out.back().last = b;
        else
            out.push_back(Piece{kind, a, b});
    };
    // single-block steps [a, b) outside the tile form: two-grid levels stay plain launches, the
    // rest becomes row programs
    auto rest = [&](size_t a, size_t b) {
        if (a >= b) return;
        bool has_coarse = false;
        for (size_t i = a; i < b; ++i) has_coarse = has_coarse || d[i].kind == StepDesc::COARSE;
        if (has_coarse) {
            push(Piece::PLAIN, a, b);
            return;
        }
        // the data-flow form needs phase ph >= 1 to gather exactly what phase ph - 1 produced,
        // so a run is cut where that chain breaks
        size_t q = a;
        while (q < b) {
            size_t q1 = q + 1;
            while (q1 < b && !(prog_granule && legacy_ok && !chains(q1))) ++q1;
            push(q1 - q >= 4 && legacy_ok ? Piece::PROGRAM : Piece::PLAIN, q, q1);
            q = q1;
        }
    };
    // steps [a, b) of eligible levels from a on (levels are whole stretches: they end inside a run)
    auto levels_end = [&](size_t a, size_t b) {
        while (a < b && d[a].level >= 0 && d[a].eligible) ++a;
        return a;
    };
    size_t k = 0;
    while (k < d.size()) {
        size_t e = k;
        // (the coarse corrections of two-grid levels sit between the single-block steps)
        while (e < d.size() && d[e].single) ++e;
        if (e == k) {
            push(Piece::KEEP, k, k + 1);
            ++k;
            continue;
        }
        if (e - k >= 4 && use_tiles && levels_end(k, e) == e && tiles_take(k, e)) {
            push(Piece::TILES, k, e);
        } else if (use_tiles && sharded) {
            // A rank with ONE level: the products between the sweeps have one op, so they are
            // single-block steps of the same run as a sweep level wherever no hand-off separates
            // them (rank 0 in front of the forward level, the last rank between the sweeps).  Every
            // stretch of levels inside the run still becomes a tile launch, the steps between them
            // stay what they were.
            size_t pend = k, c = k;
            while (c < e) {
                const size_t c2 = levels_end(c, e);
                if (c2 - c >= 4 && tiles_take(c, c2)) {
                    rest(pend, c);
                    push(Piece::TILES, c, c2);
                    pend = c = c2;
                } else {
                    c = c2 > c ? c2 : c + 1;
                }
            }
            rest(pend, e);
        } else {
            rest(k, e);
        }
        k = e;
    }
    return out;
}

}  // namespace kkt
