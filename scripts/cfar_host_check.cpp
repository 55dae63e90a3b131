// Stand-alone host program around csrc/cfar_host.h: the CA-CFAR threshold table and the argument checks of csrc/cfar.hip, meant to be
// built with -fsanitize=address,undefined and run on the CPU (tests/test_cfar_cpu.py does):
//   c++ -std=c++17 -g -fsanitize=address,undefined -I <package>/csrc scripts/cfar_host_check.cpp -o cfar_host_check && ./cfar_host_check
// Every table is filled into a heap block of exactly the length the library asks for, so a write past it is caught.
#include <math.h>
#include <stdio.h>
#include <initializer_list>
#include <stdlib.h>

#include "cfar_host.h"

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    using namespace hupr;
    int windows = 0;
    for (int g = -2; g <= 10; ++g) {
        for (int t = -2; t <= 10; ++t) {
            const int cells = cfar_window_cells(g, t);
            const bool ok = g >= 0 && t >= 1 && g + t <= kCfarMaxHalf;
            CHECK((cells > 0) == ok);
            if (!ok) {
                float one[1];
                CHECK(cfar_check_window(g, t, one, 1 << 20) != nullptr);
                CHECK(cfar_fill_alpha_table(1e-5, g, t, one, 1) == -1);
                continue;
            }
            const int w = g + t;
            CHECK(cells == (2 * w + 1) * (2 * w + 1) - (2 * g + 1) * (2 * g + 1));
            const int len = cells + 1;
            float* table = static_cast<float*>(malloc(sizeof(float) * len));
            CHECK(table);
            CHECK(cfar_check_window(g, t, table, len) == nullptr);
            CHECK(cfar_check_window(g, t, table, len - 1) != nullptr);
            CHECK(cfar_check_window(g, t, nullptr, len) != nullptr);
            CHECK(cfar_fill_alpha_table(1e-5, g, t, table, len - 1) == -1);
            for (double pfa : {1e-12, 1e-5, 1e-3, 0.5}) {
                CHECK(cfar_fill_alpha_table(pfa, g, t, table, len) == 0);
                CHECK(isinf(table[0]) && table[0] > 0);
                for (int N = 1; N < len; ++N) {
                    CHECK(isfinite(table[N]) && table[N] > 0);
                    if (N > 1) CHECK(table[N] <= table[N - 1]);
                    // the design property: (1 + alpha / N)^-N = pfa
                    const double back = pow(1.0 + cfar_alpha(pfa, N) / N, -(double)N);
                    CHECK(fabs(back / pfa - 1.0) < 1e-9);
                }
            }
            for (double pfa : {0.0, 1.0, -1.0, 2.0, (double)NAN}) CHECK(cfar_fill_alpha_table(pfa, g, t, table, len) == -1);
            free(table);
            ++windows;
        }
    }
    CHECK(windows == 36);      // g = 0..7, t = 1..8 - g
    CHECK(presence_check(1, 3, 2, 20) == nullptr && presence_check(0, 1, 1, 0) == nullptr);
    CHECK(presence_check(-1, 3, 2, 20) && presence_check(1, 0, 2, 20) && presence_check(1, 3, 0, 20) && presence_check(1, 3, 2, -1));
    printf("ok: %d windows\n", windows);
    return 0;
}
