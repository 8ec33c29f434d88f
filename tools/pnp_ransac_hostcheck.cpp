// Host check of the RANSAC stages of the device PnP (boxdreamer_amd/csrc/pnp.hip: ransac_hypothesis, ransac_final around
// pnp_wave_solve): both stages are __host__ __device__, so the 64 lanes of a "wave" run in a plain loop on the CPU (LoopRun), every
// hypothesis of a scene and then its selection and final solve, exactly what pnp_ransac_hyp_kernel / pnp_ransac_final_kernel execute.
// Built with the address and undefined-behaviour sanitizers this finds an index error in the shared state, the gathered observations
// or the workspace without a GPU.  A stand-alone program: never load it into Python.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include -c tools/pnp_ransac_hostcheck.cpp -o /tmp/pnp_ransac_hostcheck.o
//   $ROCM/lib/llvm/bin/clang++ -fsanitize=address,undefined /tmp/pnp_ransac_hostcheck.o -L$ROCM/lib -lamdhip64 -Wl,-rpath,$ROCM/lib \
//         -lpthread -o /tmp/pnp_ransac_hostcheck && /tmp/pnp_ransac_hostcheck
// (the sanitizers go to the host half only; nothing here touches a GPU)
//
// Scenes: the box (0.1, 0.07, 0.05), fx = fy = 600, c = 112, poses drawn like tests/test_gpu_pnp_wave.py's scene(); a clean round is the
// exact projections + 0.3 px normal noise, a bad round 8 uniform pixels in [30, 194]; 1000 trials (and 70, 1) from a table of 6
// distinct corners and a round for each.  Per scene it prints the trials used, the path, the inliers per round, the distance of the
// final pose from the host form (solve_one_pose) on the same observations, and the MARGIN: the smallest |error - reproj_err| over every
// scored (hypothesis, observation) pair -- a scene whose margin is below 1e-6 px could flip an inlier between two forms that differ at
// the 1e-9 level and is no test scene.  Exits non-zero when a clean round is not fully in, a bad round keeps more than one corner, the
// path is not the expected one, the pose differs from the host form by 1e-4 or more, or more than 1 scene in 10 misses the margin.
#include "../boxdreamer_amd/csrc/pnp.hip"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>

namespace {

std::mt19937_64 g_rng(7);
double normal() { static std::normal_distribution<double> d; return d(g_rng); }
double uniform01() { static std::uniform_real_distribution<double> d; return d(g_rng); }

struct Scene { std::vector<float> kp, box, K; int rounds; std::vector<int> bad; };

Scene make_scene(int rounds, std::vector<int> bad) {
    Scene s;
    s.rounds = rounds;
    s.bad = bad;
    double rv[3], t[3], R[9];
    for (int a = 0; a < 3; ++a) rv[a] = normal() * 0.9;
    t[0] = normal() * 0.05; t[1] = normal() * 0.05; t[2] = 0.6 + uniform01() * 0.4;
    rodrigues(rv, R);
    const double ext[3] = {0.1, 0.07, 0.05};
    double exact[16];
    for (int i = 0; i < 8; ++i) {
        double X[3];
        for (int a = 0; a < 3; ++a) { X[a] = ((i >> (2 - a)) & 1 ? 1.0 : -1.0) * ext[a]; s.box.push_back((float)X[a]); }
        const double pc[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1],
                              R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]};
        exact[2 * i] = pc[0] / pc[2] * 600.0 + 112.0;
        exact[2 * i + 1] = pc[1] / pc[2] * 600.0 + 112.0;
    }
    for (int r = 0; r < rounds; ++r) {
        const bool is_bad = std::find(bad.begin(), bad.end(), r) != bad.end();
        for (int i = 0; i < 16; ++i) s.kp.push_back((float)(is_bad ? 30.0 + uniform01() * 164.0 : exact[i] + normal() * 0.3));
    }
    const float K[9] = {600.f, 0, 112.f, 0, 600.f, 112.f, 0, 0, 1};
    s.K.assign(K, K + 9);
    return s;
}

std::vector<int32_t> make_picks(int rounds, int n_trials) {
    std::vector<int32_t> p;
    for (int t = 0; t < n_trials; ++t) {
        int c[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        for (int i = 0; i < 6; ++i) std::swap(c[i], c[i + (int)(uniform01() * (8 - i)) % (8 - i)]);
        for (int i = 0; i < 6; ++i) p.push_back((int32_t)(((int)(uniform01() * rounds) % rounds) * 8 + c[i]));
    }
    return p;
}

struct Tally { int scenes = 0, below_margin = 0, fails = 0; };

// expected_path: 0 (inliers), 1 (all observations), 2 (failed), -1 (any: a single trial may or may not hit clean corners)
void run_scene(const Scene& s, int n_trials, int expected_path, Tally& tally, const char* what) {
    static WaveState S;
    static RansacObs G;
    const int n_obs = s.rounds * 8;
    std::vector<int32_t> picks = make_picks(s.rounds, n_trials);
    std::vector<RansacScore> ws((size_t)n_trials);
    double margin = 1e300;
    for (int t = 0; t < n_trials; ++t)
        ransac_hypothesis(LoopRun(), S, G, s.kp.data(), s.box.data(), s.K.data(), picks.data() + (size_t)t * 6, n_obs, 2.0, 5, ws.data() + t, &margin);
    std::vector<float> pose(16, -1.f);
    std::vector<unsigned char> inl((size_t)n_obs, 7);
    float rms = -1.f;
    int32_t info[4] = {-9, -9, -9, -9};
    ransac_final(LoopRun(), S, G, s.kp.data(), s.box.data(), s.K.data(), ws.data(), n_obs, n_trials, (double)0.99f, 30, pose.data(), inl.data(), &rms, info);
    ++tally.scenes;
    bool bad = expected_path >= 0 && info[3] != expected_path;
    char rounds[64] = "";
    for (int r = 0; r < s.rounds; ++r) {
        int c = 0;
        for (int i = 0; i < 8; ++i) c += inl[(size_t)r * 8 + i];
        snprintf(rounds + strlen(rounds), sizeof rounds - strlen(rounds), "%d ", c);
        const bool is_bad = std::find(s.bad.begin(), s.bad.end(), r) != s.bad.end();
        if (expected_path == 0 && (is_bad ? c > 1 : c != 8)) bad = true;
        if (expected_path == 1 && c != 8) bad = true;
        if (expected_path == 2 && c != 0) bad = true;
    }
    // the host form (one thread, scratch arrays) on the observations the mask keeps, in index order
    std::vector<float> kp2, p32;
    for (int i = 0; i < n_obs; ++i)
        if (inl[(size_t)i]) {
            kp2.push_back(s.kp[2 * i]); kp2.push_back(s.kp[2 * i + 1]);
            for (int a = 0; a < 3; ++a) p32.push_back(s.box[(i % 8) * 3 + a]);
        }
    double d = 0.0;
    if (info[3] == 2) {
        for (int i = 0; i < 16; ++i) d = fmax(d, fabs((double)pose[i]));
        bad = bad || rms != 0.f;
    } else {
        float ref[16];
        solve_one_pose(kp2.data(), p32.data(), s.K.data(), (int)kp2.size() / 2, 30, ref);
        for (int i = 0; i < 16; ++i) d = fmax(d, fabs((double)pose[i] - ref[i]));
    }
    bad = bad || !(d < 1e-4);
    const bool low = margin < 1e-6;
    tally.below_margin += low;
    tally.fails += bad;
    printf("%-26s R %d trials %4d: used %4d best %4d inliers %2d path %d per round [%s] rms %.4f  |pose - host form| %.3g  margin %.3g px%s%s\n", what,
           s.rounds, n_trials, info[0], info[1], info[2], info[3], rounds, rms, d, margin, low ? "   (below 1e-6: no test scene)" : "", bad ? "   <-- FAIL" : "");
}

}  // namespace

int main() {
    Tally tally;
    struct Shape { int rounds; std::vector<int> bad; const char* what; };
    const Shape shapes[] = {{1, {}, "R 1 clean"}, {3, {1}, "R 3, one bad round"}, {4, {0}, "R 4, one bad round"}, {7, {2, 5}, "R 7, two bad rounds"},
                            {8, {1, 4, 6}, "R 8, three bad rounds"}, {8, {}, "R 8 clean"}};
    for (const Shape& sh : shapes)
        for (int k = 0; k < 5; ++k) run_scene(make_scene(sh.rounds, sh.bad), 1000, 0, tally, sh.what);
    for (int n_trials : {70, 1})                                 // a last batch of 6 trials; a single trial
        for (int k = 0; k < 3; ++k) {
            run_scene(make_scene(3, {1}), n_trials, n_trials == 1 ? -1 : 0, tally, "R 3, one bad round");
        }
    for (int rounds : {1, 3, 8}) {                               // every round bad: all observations
        std::vector<int> all;
        for (int r = 0; r < rounds; ++r) all.push_back(r);
        run_scene(make_scene(rounds, all), 1000, 1, tally, "every round bad");
    }
    {                                                            // a NaN corner: zeros, path 2
        Scene s = make_scene(3, {1});
        s.kp[2 * 11] = NAN;
        run_scene(s, 1000, 2, tally, "one NaN corner");
        Scene a = make_scene(8, {});
        for (auto& v : a.kp) v = NAN;
        for (auto& v : a.box) v = NAN;
        for (auto& v : a.K) v = NAN;
        run_scene(a, 70, 2, tally, "all NaN");
    }
    {                                                            // picks outside [0, n_obs): clamped, never an index out of bounds
        static WaveState S;
        static RansacObs G;
        Scene s = make_scene(3, {});
        const int32_t wild[6] = {-1, 24, 1 << 30, -(1 << 30), 23, 0};
        RansacScore sc;
        ransac_hypothesis(LoopRun(), S, G, s.kp.data(), s.box.data(), s.K.data(), wild, 24, 2.0, 5, &sc, nullptr);
        printf("picks outside the range: count %d\n", sc.count);
    }
    const bool margin_bad = tally.below_margin * 10 > tally.scenes;
    printf("%d scenes, %d below the 1e-6 px margin, %d failed\n", tally.scenes, tally.below_margin, tally.fails);
    printf(tally.fails || margin_bad ? "FAILED\n" : "all scenes: expected path and rounds, final pose within 1e-4 of the host form\n");
    return tally.fails || margin_bad ? 1 : 0;
}
