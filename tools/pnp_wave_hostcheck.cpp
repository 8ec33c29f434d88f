// Host check of the wave form of the PnP solver (boxdreamer_amd/csrc/pnp.hip: pnp_wave_solve): the driver and its phases are
// __host__ __device__, so the 64 lanes of a "wave" can be run in a plain loop on the CPU (LoopRun), phase by phase, against
// solve_one_pose (the host form).  Built with the address and undefined-behaviour sanitizers this finds an index error in the shared state without a GPU.
// A stand-alone program: never load it into Python.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -I include -c tools/pnp_wave_hostcheck.cpp -o /tmp/pnp_wave_hostcheck.o
//   $ROCM/lib/llvm/bin/clang++ -fsanitize=address,undefined /tmp/pnp_wave_hostcheck.o -L$ROCM/lib -lamdhip64 -Wl,-rpath,$ROCM/lib \
//         -lpthread -o /tmp/pnp_wave_hostcheck && /tmp/pnp_wave_hostcheck
// (the sanitizers go to the host half only; nothing here touches a GPU)
//
// Prints, per group of cases, the largest |dR|, |dt| and relative excess of the pixel RMS over the host form's, and exits non-zero when
// a pose differs from the host form by more than 1e-4, a verdict (solved / zeros) differs, or the RMS exceeds the host form's by more
// than 1e-6 relative.
#include "../boxdreamer_amd/csrc/pnp.hip"

#include <cstdio>
#include <random>

namespace {

struct Case { std::vector<float> kp, p3, K; int n; };

std::mt19937_64 g_rng(3);
double normal() { static std::normal_distribution<double> d; return d(g_rng); }
double uniform01() { static std::uniform_real_distribution<double> d; return d(g_rng); }

Case make_case(int n, const double* rv, const double* t, double fx, double fy, double cx, double cy, double noise, bool planar = false) {
    Case c;
    c.n = n;
    double R[9];
    rodrigues(rv, R);
    const double ext[3] = {0.1, 0.07, 0.05};
    for (int i = 0; i < n; ++i) {
        double X[3];
        for (int a = 0; a < 3; ++a) X[a] = i < 8 ? ((i >> (2 - a)) & 1 ? 1.0 : -1.0) * ext[a] : normal() * ext[a];
        if (planar) X[2] = 0.0;
        const double pc[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0], R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1],
                              R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]};
        for (int a = 0; a < 3; ++a) c.p3.push_back((float)X[a]);
        c.kp.push_back((float)(pc[0] / pc[2] * fx + cx + normal() * noise));
        c.kp.push_back((float)(pc[1] / pc[2] * fy + cy + normal() * noise));
    }
    const float K[9] = {(float)fx, 0, (float)cx, 0, (float)fy, (float)cy, 0, 0, 1};
    c.K.assign(K, K + 9);
    return c;
}

double pixel_rms(const Case& c, const float* pose) {
    double ss = 0.0;
    for (int i = 0; i < c.n; ++i) {
        double pc[3];
        for (int a = 0; a < 3; ++a)
            pc[a] = (double)pose[a * 4] * c.p3[i * 3] + (double)pose[a * 4 + 1] * c.p3[i * 3 + 1] + (double)pose[a * 4 + 2] * c.p3[i * 3 + 2] + pose[a * 4 + 3];
        const double du = c.kp[2 * i] - (c.K[0] * pc[0] / pc[2] + c.K[2]), dv = c.kp[2 * i + 1] - (c.K[4] * pc[1] / pc[2] + c.K[5]);
        ss += du * du + dv * dv;
    }
    return sqrt(ss / c.n);
}

struct Worst { double dR = 0, dt = 0, excess = -1e300, drms = 0; int bad = 0, solved = 0, zeros = 0; };

void run_case(const Case& c, int iters, Worst& w, const char* what) {
    float ref[16], got[16];
    solve_one_pose(c.kp.data(), c.p3.data(), c.K.data(), c.n, iters, ref);
    static WaveState S;
    double rms = 0.0;
    const bool ok = pnp_wave_solve(LoopRun(), S, c.kp.data(), c.p3.data(), c.K.data(), c.n, iters, &rms);
    for (int i = 0; i < 16; ++i) got[i] = ok ? S.out[i] : 0.f;
    const bool ref_ok = ref[15] == 1.f;
    if (ok != ref_ok) { printf("  VERDICT differs (%s): wave %d host %d\n", what, (int)ok, (int)ref_ok); ++w.bad; return; }
    if (!ok) { ++w.zeros; return; }
    ++w.solved;
    bool finite = true;
    for (int i = 0; i < 12; ++i) finite = finite && finite_d(got[i]) == finite_d(ref[i]);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) w.dR = fmax(w.dR, fabs((double)got[i * 4 + j] - ref[i * 4 + j]));
        w.dt = fmax(w.dt, fabs((double)got[i * 4 + 3] - ref[i * 4 + 3]));
    }
    const double r_ref = pixel_rms(c, ref), r_got = pixel_rms(c, got);
    w.excess = fmax(w.excess, r_got / fmax(r_ref, 1e-3) - 1.0);
    w.drms = fmax(w.drms, fabs((float)rms - r_got) / fmax(r_got, 1e-3));
    if (!finite || !(r_got <= r_ref * (1 + 1e-6) || r_got < 1e-3)) { printf("  RMS above the host form's (%s): %.9g vs %.9g\n", what, r_got, r_ref); ++w.bad; }
}

int report(const char* name, const Worst& w) {
    printf("%-28s solved %3d zeros %2d  max|dR| %.3g  max|dt| %.3g  rms excess %.3g  rms_px vs recomputed %.3g%s\n", name, w.solved, w.zeros, w.dR,
           w.dt, w.excess, w.drms, (w.bad || w.dR >= 1e-4 || w.dt >= 1e-4 || w.drms >= 1e-4) ? "   <-- FAIL" : "");
    return (w.bad || w.dR >= 1e-4 || w.dt >= 1e-4 || w.drms >= 1e-4) ? 1 : 0;
}

void random_pose(double* rv, double* t) {
    for (int a = 0; a < 3; ++a) rv[a] = normal() * 0.9;
    t[0] = normal() * 0.05; t[1] = normal() * 0.05; t[2] = 0.6 + uniform01() * 0.4;
}

}  // namespace

int main() {
    int fails = 0;
    double rv[3], t[3];
    {
        Worst w;
        for (int n : {6, 7, 8, 9, 16, 24, 63, 64})
            for (int k = 0; k < 5; ++k) { random_pose(rv, t); run_case(make_case(n, rv, t, 600, 600, 112, 112, 0.7), 30, w, "point counts"); }
        fails += report("point counts 6..64", w);
    }
    {
        Worst w;
        for (int k = 0; k < 40; ++k) { random_pose(rv, t); run_case(make_case(8, rv, t, 600, 600, 112, 112, 0.7), 30, w, "batch"); }
        fails += report("40 poses, 8 points", w);
    }
    {
        Worst w;
        const double t0[3] = {0.01, 0.02, 0.7}, pi = 3.14159265358979323846;
        for (double ang : {pi - 1e-2, pi - 1e-5, pi})
            for (double noise : {0.0, 0.7}) {
                const double r[3] = {0.6 * ang, 0.0, 0.8 * ang};
                run_case(make_case(8, r, t0, 600, 600, 112, 112, noise), 30, w, "near pi");
            }
        const double zero[3] = {0, 0, 0};
        run_case(make_case(8, zero, t0, 600, 600, 112, 112, 0.0), 30, w, "identity");
        fails += report("near pi, identity", w);
    }
    {
        Worst w;
        for (int k = 0; k < 5; ++k) { random_pose(rv, t); run_case(make_case(8, rv, t, 640, 480, 100, 120, 0.7), 30, w, "fx != fy"); }
        fails += report("fx 640 fy 480", w);
    }
    for (int iters : {0, 1, 2}) {
        Worst w;
        for (int k = 0; k < 5; ++k) { random_pose(rv, t); run_case(make_case(8, rv, t, 600, 600, 112, 112, 0.7), iters, w, "iters"); }
        char name[32];
        snprintf(name, sizeof name, "iters = %d", iters);
        fails += report(name, w);
    }
    {
        Worst w;
        random_pose(rv, t);
        Case c = make_case(8, rv, t, 600, 600, 112, 112, 0.0);
        for (auto& v : c.kp) v = 112.f;
        run_case(c, 30, w, "one pixel");
        random_pose(rv, t);
        run_case(make_case(8, rv, t, 600, 600, 112, 112, 0.7, true), 30, w, "planar");
        c = make_case(8, rv, t, 600, 600, 112, 112, 0.7);
        c.kp[3 * 2] = NAN;
        run_case(c, 30, w, "NaN corner");
        c = make_case(8, rv, t, 600, 600, 112, 112, 0.7);
        c.K[0] = NAN;
        run_case(c, 30, w, "NaN K");
        c = make_case(64, rv, t, 600, 600, 112, 112, 0.7);
        for (auto& v : c.kp) v = NAN;
        for (auto& v : c.p3) v = NAN;
        for (auto& v : c.K) v = NAN;
        run_case(c, 30, w, "all NaN");
        c = make_case(8, rv, t, 600, 600, 112, 112, 0.7);
        c.p3[5] = NAN;                                   // a NaN that passes the input check: 60 sweeps, then the residual check
        run_case(c, 30, w, "NaN 3-D point");
        fails += report("degenerate / NaN", w);
    }
    printf(fails ? "FAILED\n" : "all groups within 1e-4 of the host form, rms <= host rms (1 + 1e-6)\n");
    return fails ? 1 : 0;
}
