// Host side of the CA-CFAR detector (cfar.hip): the window's cell count, the threshold table and the argument checks.  Plain C++
// without the HIP runtime, so that a stand-alone host program can be built around it (scripts/cfar_host_check.cpp).
#pragma once
#include <math.h>
#include <stddef.h>

namespace hupr {

constexpr int kCfarMaxHalf = 8;      // largest guard + train: the 17 x 17 window

// Training cells of an interior cell: (2 w + 1)^2 - (2 g + 1)^2 with w = guard + train; 0 for a window the detector refuses.
inline int cfar_window_cells(int guard, int train) {
    if (guard < 0 || train < 1 || guard > kCfarMaxHalf || train > kCfarMaxHalf || guard + train > kCfarMaxHalf) return 0;
    const int w = guard + train;
    return (2 * w + 1) * (2 * w + 1) - (2 * guard + 1) * (2 * guard + 1);
}

// The exact cell-averaging factor for exponentially distributed cells: alpha[N] = N (pfa^(-1/N) - 1), written through expm1 so that
// a large N loses no digits.
inline double cfar_alpha(double pfa, int N) { return (double)N * expm1(-log(pfa) / (double)N); }

// What is wrong with a detector call's window and table, or null.
inline const char* cfar_check_window(int guard, int train, const void* alpha_table, int table_len) {
    if (guard < 0) return "guard is negative";
    if (train < 1) return "train is below 1";
    if (guard > kCfarMaxHalf || train > kCfarMaxHalf || guard + train > kCfarMaxHalf) return "guard + train exceeds 8";
    if (!alpha_table) return "null alpha table";
    if (table_len < cfar_window_cells(guard, train) + 1) return "the alpha table is shorter than the window needs";
    return nullptr;
}

// table[0] = +inf (no training cell: never a detection), table[N] = (float)alpha[N] for N = 1 .. len - 1.  -> 0, or -1 for a bad
// argument (pfa outside (0, 1), a refused window, a null table, len shorter than the window needs).
inline int cfar_fill_alpha_table(double pfa, int guard, int train, float* table, int len) {
    if (!(pfa > 0.0 && pfa < 1.0)) return -1;
    if (cfar_check_window(guard, train, table, len)) return -1;
    table[0] = INFINITY;
    for (int N = 1; N < len; ++N) table[N] = (float)cfar_alpha(pfa, N);
    return 0;
}

// What is wrong with a presence-gate call's settings, or null.
inline const char* presence_check(int lanes, int min_cells, int confirm, int hold) {
    if (lanes < 0) return "lanes is negative";
    if (min_cells < 1) return "min_cells is below 1";
    if (confirm < 1) return "confirm is below 1";
    if (hold < 0) return "hold is negative";
    return nullptr;
}

}  // namespace hupr
