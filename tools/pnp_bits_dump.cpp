// Bit dump of the host side of the PnP solver (boxdreamer_amd/csrc/pnp.hip), for comparing two versions of that file: the thread
// driver (solve_one_pose), the wave driver under the loop runner (pnp_wave_solve with LoopRun: pose and rms) and both RANSAC host stages
// (ransac_hypothesis: every score; ransac_final: pose, inliers, rms, info) on seeded scenes, every output printed as hex.  The host
// half is compiled without FMA contraction, so two versions that do the same arithmetic in the same order print the same bytes: build
// this once per version (PNP_SOURCE names the file to include, by default the tree's) with the library's own flags and compare.
// A stand-alone program: never load it into Python.
//
//   hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 -I include [-DPNP_SOURCE='"/path/to/other/pnp.hip"'] \
//         -c tools/pnp_bits_dump.cpp -o /tmp/pnp_bits_dump.o
//   $ROCM/lib/llvm/bin/clang++ /tmp/pnp_bits_dump.o -L$ROCM/lib -lamdhip64 -Wl,-rpath,$ROCM/lib -lpthread -o /tmp/pnp_bits_dump
//   /tmp/pnp_bits_dump > a.txt          (and the other build > b.txt; cmp a.txt b.txt)
// (nothing here touches a GPU)
//
// Scenes: 6 to 64 points, 0 to 7.5 px of noise, fx != fy, a box 8 m away, a 2 mm-thin box, rotations at pi and pi - 1e-5, a NaN corner,
// a NaN in K, a NaN 3-D point; every solver scene at iters 0, 5 and 400.
#ifndef PNP_SOURCE
#define PNP_SOURCE "../boxdreamer_amd/csrc/pnp.hip"
#endif
#include PNP_SOURCE

#include <cstdio>
#include <cstring>
#include <random>

namespace {

std::mt19937_64 g_rng(20261021);
double normal() { static std::normal_distribution<double> d; return d(g_rng); }
double uniform01() { static std::uniform_real_distribution<double> d; return d(g_rng); }

struct Scene { std::vector<float> kp, p3, K; int n; };

// n points (the 8 box corners first, then normal * ext) under the pose (rv, t), noise in pixels
Scene make_scene(int n, const double* rv, const double* t, const double* ext, double fx, double fy, double noise) {
    Scene s;
    s.n = n;
    double R[9];
    rodrigues(rv, R);
    for (int i = 0; i < n; ++i) {
        double X[3];
        for (int a = 0; a < 3; ++a) X[a] = (i < 8 ? ((i >> (2 - a)) & 1 ? 1.0 : -1.0) : normal()) * ext[a];
        const double pc[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1],
                              R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]};
        for (int a = 0; a < 3; ++a) s.p3.push_back((float)X[a]);
        s.kp.push_back((float)(pc[0] / pc[2] * fx + 112.0 + normal() * noise));
        s.kp.push_back((float)(pc[1] / pc[2] * fy + 112.0 + normal() * noise));
    }
    const float K[9] = {(float)fx, 0, 112.f, 0, (float)fy, 112.f, 0, 0, 1};
    s.K.assign(K, K + 9);
    return s;
}

void hex32(const void* p, int count) {
    for (int i = 0; i < count; ++i) { uint32_t u; memcpy(&u, (const char*)p + 4 * i, 4); printf(" %08x", u); }
}
void hex64(const void* p, int count) {
    for (int i = 0; i < count; ++i) { unsigned long long u; memcpy(&u, (const char*)p + 8 * i, 8); printf(" %016llx", u); }
}

int g_scene = 0, g_solved[2] = {0, 0}, g_zeros[2] = {0, 0};

void dump_solvers(const Scene& s, const char* what) {
    static WaveState S;
    for (int iters : {0, 5, 400}) {
        float pose[16];
        solve_one_pose(s.kp.data(), s.p3.data(), s.K.data(), s.n, iters, pose);
        printf("%d %s n %d iters %d thread", g_scene, what, s.n, iters);
        hex32(pose, 16);
        ++(pose[15] == 1.f ? g_solved : g_zeros)[0];
        double rms = 0.0;
        const bool ok = pnp_wave_solve(LoopRun(), S, s.kp.data(), s.p3.data(), s.K.data(), s.n, iters, &rms);
        printf("\n%d %s n %d iters %d wave %d", g_scene, what, s.n, iters, (int)ok);
        if (ok) { hex32(S.out, 16); hex64(&rms, 1); }
        ++(ok ? g_solved : g_zeros)[1];
        printf("\n");
    }
    ++g_scene;
}

// R rounds of the 8 corners; the rounds listed in `bad` hold uniform pixels.  n_trials hypotheses from a seeded table of picks.
void dump_ransac(int rounds, std::vector<int> bad, double noise, int n_trials, int nan_obs, const char* what) {
    static WaveState S;
    static RansacObs G;
    const double ext[3] = {0.1, 0.07, 0.05};
    double rv[3], t[3];
    for (int a = 0; a < 3; ++a) rv[a] = normal() * 0.9;
    t[0] = normal() * 0.05; t[1] = normal() * 0.05; t[2] = 0.6 + uniform01() * 0.4;
    std::vector<float> kp, box, K;
    for (int r = 0; r < rounds; ++r) {
        const Scene s = make_scene(8, rv, t, ext, 600, 600, noise);
        bool is_bad = false;
        for (int b : bad) is_bad = is_bad || b == r;
        for (int i = 0; i < 16; ++i) kp.push_back(is_bad ? (float)(30.0 + uniform01() * 164.0) : s.kp[i]);
        if (r == 0) { box = s.p3; K = s.K; }
    }
    const int n_obs = rounds * 8;
    if (nan_obs >= 0) kp[2 * nan_obs] = NAN;
    std::vector<int32_t> picks;
    for (int i = 0; i < n_trials * 6; ++i) picks.push_back((int32_t)(uniform01() * n_obs) % n_obs);
    std::vector<RansacScore> ws((size_t)n_trials);
    for (int tr = 0; tr < n_trials; ++tr) {
        ransac_hypothesis(LoopRun(), S, G, kp.data(), box.data(), K.data(), picks.data() + (size_t)tr * 6, n_obs, 2.0, 5, ws.data() + tr, nullptr);
        printf("%d %s R %d hyp %d count %d mask %016llx err", g_scene, what, rounds, tr, ws[tr].count, ws[tr].mask);
        hex64(&ws[tr].err_sum, 1);
        printf("\n");
    }
    for (int iters : {5, 400}) {
        float pose[16], rms = -1.f;
        std::vector<unsigned char> inl((size_t)n_obs, 7);
        int32_t info[4] = {-9, -9, -9, -9};
        ransac_final(LoopRun(), S, G, kp.data(), box.data(), K.data(), ws.data(), n_obs, n_trials, (double)0.99f, iters, pose, inl.data(), &rms, info);
        printf("%d %s R %d final iters %d info %d %d %d %d rms", g_scene, what, rounds, iters, info[0], info[1], info[2], info[3]);
        hex32(&rms, 1);
        printf(" pose");
        hex32(pose, 16);
        printf(" inliers ");
        for (unsigned char c : inl) printf("%d", (int)c);
        printf("\n");
    }
    ++g_scene;
}

}  // namespace

int main() {
    const double box[3] = {0.1, 0.07, 0.05}, thin[3] = {0.075, 0.035, 0.002}, pi = 3.14159265358979323846;
    double rv[3], t[3];
    auto random_pose = [&](double depth) {
        for (int a = 0; a < 3; ++a) rv[a] = normal() * 0.9;
        t[0] = normal() * 0.0625 * depth; t[1] = normal() * 0.0625 * depth; t[2] = depth;
    };
    for (int n : {6, 7, 8, 9, 16, 33, 63, 64})
        for (double noise : {0.0, 0.7, 3.0, 7.5})
            for (int k = 0; k < 10; ++k) { random_pose(0.55 + uniform01() * 0.5); dump_solvers(make_scene(n, rv, t, box, 600, 600, noise), "points"); }
    for (double noise : {0.0, 0.7, 5.0})
        for (int k = 0; k < 8; ++k) {
            random_pose(0.55 + uniform01() * 0.5);
            dump_solvers(make_scene(8, rv, t, box, 640, 450, noise), "aniso");
            random_pose(8.0);
            dump_solvers(make_scene(8, rv, t, box, 600, 600, noise), "far");
            random_pose(0.4 + uniform01() * 0.3);
            dump_solvers(make_scene(8, rv, t, thin, 600, 600, noise), "thin");
            for (int a = 0; a < 3; ++a) rv[a] = normal() * 3.0;
            dump_solvers(make_scene(16, rv, t, box, 600, 600, noise), "big_rot");
        }
    for (double ang : {pi, pi - 1e-5})
        for (double noise : {0.0, 0.7})
            for (int k = 0; k < 4; ++k) {
                double axis[3] = {normal(), normal(), normal()};
                if (k == 0) { axis[0] = 0.6; axis[1] = 0.0; axis[2] = 0.8; }
                const double len = sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
                const double r[3] = {axis[0] / len * ang, axis[1] / len * ang, axis[2] / len * ang}, t0[3] = {0.01, 0.02, 0.7};
                dump_solvers(make_scene(8, r, t0, box, 600, 600, noise), "near_pi");
            }
    for (int k = 0; k < 3; ++k) {
        random_pose(0.7);
        Scene s = make_scene(8 + 28 * k, rv, t, box, 600, 600, 0.7);
        s.kp[2 * 3] = NAN;
        dump_solvers(s, "nan_corner");
        s = make_scene(8 + 28 * k, rv, t, box, 600, 600, 0.7);
        s.K[4 * (k % 2)] = NAN;
        dump_solvers(s, "nan_K");
        s = make_scene(8 + 28 * k, rv, t, box, 600, 600, 0.7);
        s.p3[5] = NAN;
        dump_solvers(s, "nan_point");
    }
    const int solver_scenes = g_scene;
    for (int k = 0; k < 3; ++k) {
        dump_ransac(1, {}, 0.3, 40, -1, "ransac_clean");
        dump_ransac(3, {1}, 0.3, 70, -1, "ransac_one_bad");
        dump_ransac(8, {1, 4, 6}, 0.7, 100, -1, "ransac_three_bad");
        dump_ransac(8, {}, 7.5, 40, -1, "ransac_noisy");
        dump_ransac(2, {0, 1}, 0.3, 40, -1, "ransac_all_bad");
        dump_ransac(3, {1}, 0.3, 40, 11, "ransac_nan_corner");
    }
    fprintf(stderr, "%d solver scenes x 3 iteration counts: thread form solved %d zeros %d, wave form solved %d zeros %d; %d RANSAC scenes\n",
            solver_scenes, g_solved[0], g_zeros[0], g_solved[1], g_zeros[1], g_scene - solver_scenes);
    return 0;
}
