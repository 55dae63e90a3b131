// Stand-alone host program around csrc/radar_points_host.h: the argument checks of hupr_radar_peaks_f32 and hupr_radar_points_fuse_f32
// and the geometry the fuse entry derives, meant to be built with -fsanitize=address,undefined and run on the CPU
// (tests/test_radar_points_cpu.py does):
//   c++ -std=c++17 -g -fsanitize=address,undefined -I <package>/csrc scripts/radar_points_host_check.cpp -o check && ./check
// Every geometry lives in a heap block of exactly the 14 doubles the library reads, so a read past it is caught.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "radar_points_host.h"

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
            return 1;                                                 \
        }                                                             \
    } while (0)

static double* geometry(const double* a_h, const double* a_v) {
    double* g = static_cast<double*>(malloc(sizeof(double) * hupr::kFuseGeometryLen));
    if (!g) return nullptr;
    const double o_h[3] = {0.02, 0.0, 0.01}, o_v[3] = {0.0, 0.0, -0.10};
    g[0] = 0.0375;
    g[1] = 0.1015625;
    memcpy(g + 2, a_h, sizeof(double) * 3);
    memcpy(g + 5, o_h, sizeof(double) * 3);
    memcpy(g + 8, a_v, sizeof(double) * 3);
    memcpy(g + 11, o_v, sizeof(double) * 3);
    return g;
}

int main() {
    using namespace hupr;
    int settings = 0;
    for (int mp = -1; mp <= 258; ++mp)
        for (int sr = -1; sr <= 5; ++sr)
            for (int sa = -1; sa <= 9; ++sa) {
                const bool ok = mp >= 1 && mp <= 256 && sr >= 0 && sr <= 4 && sa >= 0 && sa <= 8;
                CHECK((peaks_check(3, mp, sr, sa) == nullptr) == ok);
                CHECK(peaks_check(-1, mp, sr, sa) != nullptr);
                settings += ok;
            }
    CHECK(settings == 256 * 5 * 9);
    CHECK(peaks_check(0, 64, 1, 4) == nullptr);

    const double x[3] = {1, 0, 0}, y[3] = {0, 1, 0}, z[3] = {0, 0, 1}, mz[3] = {0, 0, -1}, skew[3] = {0.6, 0.0, 0.8}, longer[3] = {1.1, 0, 0};
    FuseGeometry g;
    double* geo = geometry(x, z);
    CHECK(geo);
    CHECK(fuse_check(2, 64, 32, geo, 1.5, 1, &g) == nullptr);
    CHECK(g.b[0] == 0.0 && g.b[1] == 1.0 && g.b[2] == 0.0);                    // z x x = y
    CHECK(g.oh_ah == 0.02 && g.ov_av == -0.10 && g.oh_av == 0.01 && g.oh_b == 0.0);
    CHECK(g.range_bin_m == 0.0375 && g.doppler_mps_per_bin == 0.1015625);
    CHECK(fuse_check(2, 64, 32, geo, 1.5, 1, nullptr) == nullptr);
    CHECK(fuse_check(-1, 64, 32, geo, 1.5, 1, &g) && fuse_check(2, 0, 32, geo, 1.5, 1, &g) && fuse_check(2, 64, 257, geo, 1.5, 1, &g));
    CHECK(fuse_check(2, 64, 32, geo, -0.5, 1, &g) && fuse_check(2, 64, 32, geo, NAN, 1, &g) && fuse_check(2, 64, 32, geo, INFINITY, 1, &g));
    CHECK(fuse_check(2, 64, 32, geo, 1.5, -1, &g) && fuse_check(2, 64, 32, geo, 1.5, 8, &g) && fuse_check(2, 64, 32, nullptr, 1.5, 1, &g));
    for (int i = 0; i < kFuseGeometryLen; ++i) {
        const double keep = geo[i];
        geo[i] = NAN;
        CHECK(fuse_check(2, 64, 32, geo, 1.5, 1, &g) != nullptr);
        geo[i] = INFINITY;
        CHECK(fuse_check(2, 64, 32, geo, 1.5, 1, &g) != nullptr);
        geo[i] = keep;
    }
    geo[0] = 0.0;
    CHECK(fuse_check(2, 64, 32, geo, 1.5, 1, &g) != nullptr);
    geo[0] = 0.0375;
    geo[1] = -1.0;
    CHECK(fuse_check(2, 64, 32, geo, 1.5, 1, &g) != nullptr);
    free(geo);

    geo = geometry(x, mz);                                                     // the vertical array mounted the other way: b flips to +y
    CHECK(geo && fuse_check(1, 1, 1, geo, 0.0, 0, &g) == nullptr && g.b[1] == 1.0 && g.ov_av == 0.10);
    free(geo);
    geo = geometry(skew, y);                                                   // b = y x skew has no y component
    CHECK(geo && fuse_check(1, 1, 1, geo, 1.5, 1, &g) != nullptr);
    free(geo);
    geo = geometry(x, skew);                                                   // not orthogonal
    CHECK(geo && fuse_check(1, 1, 1, geo, 1.5, 1, &g) != nullptr);
    free(geo);
    geo = geometry(longer, z);                                                 // no unit vector
    CHECK(geo && fuse_check(1, 1, 1, geo, 1.5, 1, &g) != nullptr);
    free(geo);
    printf("ok: %d settings\n", settings);
    return 0;
}
