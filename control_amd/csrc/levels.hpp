// The time levels a rank of a device re-linearisation plan holds, trades and downloads (relin.hpp,
// reaction.hpp).  Host-only and free of HIP and of the rest of the library:
// tests/native/level_windows.cpp prints these numbers in a program of its own.
#pragma once

namespace kkt {

struct LevelRange {   // half-open, global levels
    int l0, l1;
};

// The rank owns the block rows [lo, lo + nl) of both families (one rank: all m) and holds the
// levels its rows read: v from level v_l0 (v_n of them), zeta from z_l0, D and the element matrices
// from D_l0; everything per block (p, mu, the data rows) is the owned blocks'.
//   BE  v [lo - 1, hi)   zeta [lo, hi]   D [lo, hi)    (level -1 and level n_t do not exist)
//   CN  v [lo, hi]       zeta [lo, hi]   D [lo, hi]
// (BE's block i is (v_i, zeta_i), CN's (v_{i+1}, zeta_i).)  The levels outside the rank's own are
// halos: v's first from the rank below, zeta's last from the rank above (exchange_iterate_halos,
// compose.hpp), CN's D_lo assembled here from the halo v.  The stationary plan is BE with
// n_t = 1: every window [0, 1), no halo.
struct LevelWindows {
    int n_t = 0, m = 0;   // global: time levels, unknown blocks per family
    bool CN = false;
    int lo = 0, nl = 0, v_l0 = 0, v_n = 0, z_l0 = 0, z_n = 0, D_l0 = 0, D_n = 0;
    bool v_halo = false, z_halo = false;   // the first v / last zeta level belongs to a neighbour

    int hi() const { return lo + nl; }
    // the ranks the halos are traded with: zeta's last level comes from `up` and v's last owned
    // level goes there, v's first level comes from `dn` and zeta's first goes there; -1: nobody
    int up(int rank) const { return z_halo ? rank + 1 : -1; }
    int dn(int rank) const { return v_halo ? rank - 1 : -1; }
    // slot in the v window of the last owned v level (BE level hi - 1, CN level hi)
    int v_last_slot() const { return hi() - (CN ? 0 : 1) - v_l0; }
    // What an upload takes from the global arrays: the windows, halo levels included.  What a
    // download writes (`owned`): the levels of the rank's blocks (CN: v one level up), and the
    // fixed levels -- CN's v_0, zeta of the last level -- on the rank whose window holds them.
    LevelRange v_levels(bool owned) const {
        if (!owned) return {v_l0, v_l0 + v_n};
        return CN ? LevelRange{lo == 0 ? 0 : lo + 1, hi() + 1} : LevelRange{lo, hi()};
    }
    LevelRange z_levels(bool owned) const {
        if (!owned) return {z_l0, z_l0 + z_n};
        return {lo, CN && hi() == m ? hi() + 1 : hi()};
    }
    // [v_l0, v_end, z_l0, z_end, D_l0, D_end, lo, hi), half-open ranges
    void report(int out[8]) const {
        const int w[8] = {v_l0, v_l0 + v_n, z_l0, z_l0 + z_n, D_l0, D_l0 + D_n, lo, hi()};
        for (int k = 0; k < 8; ++k) out[k] = w[k];
    }
};

// The windows of the block rows [lo, hi) of n_t levels (one rank: lo = 0, hi = m).
inline LevelWindows level_windows(int n_t, bool cn, int lo, int hi) {
    LevelWindows w;
    w.n_t = n_t;
    w.CN = cn;
    w.m = cn ? n_t - 1 : n_t;
    w.lo = w.z_l0 = w.D_l0 = lo;
    w.nl = hi - lo;
    w.v_halo = lo > 0;
    w.z_halo = hi < w.m;
    w.v_l0 = cn ? lo : lo - (int)w.v_halo;
    w.v_n = (cn ? hi + 1 : hi) - w.v_l0;
    w.z_n = w.nl + (cn ? 1 : (int)w.z_halo);
    w.D_n = cn ? w.nl + 1 : w.nl;
    return w;
}

}  // namespace kkt
