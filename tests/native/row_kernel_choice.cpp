// The kernel-choice functions of control_amd/csrc/kernels.hpp (rows_kernel, shared_kernel,
// il_kernel) against the table the launchers of kernels.hip implemented as switch statements
// before they dispatched on these functions.  The table below is written out from those switches;
// nothing in it is computed with the functions under test.  Host-only: HIP's headers are read
// for the types of kernels.hpp, its library is not linked.
#include <cstdio>

#include "../../control_amd/csrc/kernels.hpp"

using namespace kkt;

static int failures = 0;

static void expect(const char *what, int a, int b, int c, int d, const RowKernel &k,
                   RowFamily family, int width, bool declined) {
    if (k.family == family && k.width == width && k.declined == declined) return;
    ++failures;
    std::printf("%s(%d, %d, %d, %d): family %d width %d declined %d, expected %d %d %d\n", what, a, b,
                c, d, (int)k.family, k.width, (int)k.declined, (int)family, width, (int)declined);
}

int main() {
    const int widths[] = {-4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12,
                          13, 14, 15, 16, 17, 20, 24, 38};
    // launch_rowops, tag 1: `if (R != 2) launch_one<1, 0>`; `switch (uniform_w)` with the cases
    // 1 .. 16 -> launch_one<2, n>, every other value (the ragged tags -2, -3, -4 with tag != 0
    // too) -> launch_one<2, 0>; launch_one: pc_row_step if h_single (cleared unless nops == 1)
    for (int R = 1; R <= 2; ++R)
        for (int w : widths)
            for (int nops : {1, 2, 5})
                for (int single = 0; single <= 1; ++single) {
                    int width = 0;
                    if (R == 2) switch (w) {
                        case 1: case 2: case 3: case 4: case 5: case 6: case 7: case 8:
                        case 9: case 10: case 11: case 12: case 13: case 14: case 15: case 16:
                            width = w;
                            break;
                        default: width = 0;
                    }
                    const bool step = single && nops == 1;
                    expect("rows_kernel", R, w, nops, single, rows_kernel(R, w, nops, single != 0),
                           step ? ROW_PC_ROW_STEP : ROW_PC_ROWS, width, false);
                }
    // launch_rowops_shared: `if (R != 2 || nops < 4) return false`; `switch (uniform_w)` with the
    // cases 1 .. 8 -> pc_rows_shared<n, 4>, default -> pc_rows_shared_g<4, 4>
    for (int R = 1; R <= 2; ++R)
        for (int w : widths)
            for (int nops : {0, 1, 2, 3, 4, 5, 8, 64}) {
                const bool declined = R == 1 || nops == 0 || nops == 1 || nops == 2 || nops == 3;
                bool fixed = false;
                switch (w) {
                    case 1: case 2: case 3: case 4: case 5: case 6: case 7: case 8: fixed = true;
                }
                expect("shared_kernel", R, w, nops, 0, shared_kernel(R, w, nops),
                       fixed ? ROW_PC_ROWS_SHARED : ROW_PC_ROWS_SHARED_G, fixed ? w : 4, declined);
            }
    // launch_rowops_il: `if (uniform_w > 0 && uniform_w <= 8) pc_rows_il<8> else pc_rows_il<4>`
    for (int w : widths) {
        const bool eight = w == 1 || w == 2 || w == 3 || w == 4 || w == 5 || w == 6 || w == 7 || w == 8;
        expect("il_kernel", w, 0, 0, 0, il_kernel(w), ROW_PC_ROWS_IL, eight ? 8 : 4, false);
    }
    // the families are the values include/kkt.h reports (KKT_ROWSTEP_PC_*)
    if (ROW_PC_ROWS != 0 || ROW_PC_ROW_STEP != 1 || ROW_PC_ROWS_SHARED != 2 ||
        ROW_PC_ROWS_SHARED_G != 3 || ROW_PC_ROWS_IL != 4)
        ++failures;
    std::printf("row kernel choice: %d failures\n", failures);
    return failures ? 1 : 0;
}
