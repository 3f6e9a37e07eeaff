// The level windows of the device re-linearisation plans (control_amd/csrc/levels.hpp) as the
// library computes them, printed: for every group `n_t cn lo hi rank` of the command line one line
//   window <the eight numbers of report()> halo <v_halo> <z_halo> neighbours <up> <dn>
//   v_last <slot> owned <v begin> <v end> <zeta begin> <zeta end>
// A program of its own (tests/test_level_windows.py builds it plain and under the address and
// undefined-behaviour sanitizers and compares every line with tests/reaction_shard_ref.py): no GPU,
// no HIP, nothing of the library but the header.
#include <cstdio>
#include <cstdlib>

#include "../../control_amd/csrc/levels.hpp"

int main(int argc, char **argv) {
    if (argc < 6 || (argc - 1) % 5 != 0) {
        std::fprintf(stderr, "usage: %s n_t cn lo hi rank [n_t cn lo hi rank ...]\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 4 < argc; a += 5) {
        const int n_t = std::atoi(argv[a]), cn = std::atoi(argv[a + 1]), lo = std::atoi(argv[a + 2]),
                  hi = std::atoi(argv[a + 3]), rank = std::atoi(argv[a + 4]);
        const kkt::LevelWindows w = kkt::level_windows(n_t, cn != 0, lo, hi);
        int r[8];
        w.report(r);
        const kkt::LevelRange v = w.v_levels(true), z = w.z_levels(true);
        std::printf("window %d %d %d %d %d %d %d %d halo %d %d neighbours %d %d v_last %d "
                    "owned %d %d %d %d\n",
                    r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], (int)w.v_halo, (int)w.z_halo,
                    w.up(rank), w.dn(rank), w.v_last_slot(), v.l0, v.l1, z.l0, z.l1);
        // the upload ranges are the windows
        const kkt::LevelRange vw = w.v_levels(false), zw = w.z_levels(false);
        if (vw.l0 != r[0] || vw.l1 != r[1] || zw.l0 != r[2] || zw.l1 != r[3] || w.hi() != r[7] ||
            w.n_t != n_t || w.m != (cn ? n_t - 1 : n_t)) {
            std::printf("FAILED: the upload ranges are not the reported windows\n");
            return 1;
        }
    }
    return 0;
}
