// Pose from the decoded box corners on the GPU ("next" row f3 of SURVEY.md section 8): the reference solves one
// cv2.solvePnP(SOLVEPNP_ITERATIVE) per sample in a Python loop on the host (src/models/utils/box_utils.py:139-199).
// This kernel restates the same published algorithm as boxdreamer_amd/pnp.py -- DLT initialisation for non-planar
// points, then Levenberg-Marquardt on the reprojection error over (rvec, tvec) with a forward-difference Jacobian --
// one thread per pose in fp64, so the 8 corners never leave the device and the per-batch host solve (9 ms per 32
// poses) disappears from the serving loop.  The work is tiny (~2e5 flops per pose) and latency-bound: no attempt is
// made to spread one pose over a wavefront.  PARITY against OpenCV is un-pinned (no cv2 in the image); the kernel is
// tested against the numpy form, which it follows step by step.
// That is the THREAD form (bd_solve_pnp): its per-thread arrays live in scratch memory and 32 poses are half a wavefront on one CU.  The
// WAVE form (bd_solve_pnp_wave, pnp_wave_kernel below) gives every pose a wavefront and a workgroup of its own: the same algorithm with the
// state in LDS, the 12 x 12 eigen-problem as 6 simultaneous rotations per step and the Jacobian's six perturbed poses side by side.
// The RANSAC form (bd_solve_pnp_ransac_wave, further below) runs that solver once per hypothesis: the dense multi-round pose.
// WHAT IS PINNED: tests/test_pnp_regimes_host.py and tests/test_gpu_pnp_regimes.py run every form, host and device, over a table of
// regimes (metres and millimetres, a tight crop's intrinsics, a close-up, rotations past pi, 64 points, 3 / 5 / 8 px of noise, a
// nearly planar box, a box 15 px across) against an independent fp64 minimiser of the pixel error.  In the well-posed regimes every form
// reaches that minimum and the forms agree to 1e-4 (measured: ~1e-7, the fp32 output).  In the hard ones (thin, noise5, noise8, far) a
// returned pose is stationary and in front of the camera, and up to 5 % may sit in another local minimum of the DLT start.  The forms
// are the same rules throughout, and the native forms share their text -- the DLT start with its repairs (dlt_start: the proper rotation
// after a sign flip, depth_clear) and the LM rule (lm_propose, lm_accept, lm_finish: the stop rule lm_converged, the accept test, the
// front test); the drivers (solve_one_pose, pnp_wave_solve) differ in the 12 x 12 eigen-solver and in how the per-point sums are spread
// over lanes -- but NOT the same bits: the 12 x 12 null vector comes from a cyclic Jacobi sweep here, a round-robin
// one in the wave form and LAPACK's SVD in numpy, and a last-bit difference at an accept / reject decision is amplified in the hard
// regimes, where two forms may then settle in different minima.  (Before these tests the forms DID part systematically there: the
// sign of the null vector, which each eigen-solver chooses freely, decided whether the "points in front" repair produced a proper
// rotation or a reflection, and LM then spent its iterations leaving the reflection's rotation vector.)
#include "bd_common.h"
#include <cmath>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <functional>
#include <unistd.h>
#include <vector>
#include <memory>
#include <climits>

namespace {

constexpr int MAXPTS = 64;

// (isfinite is a __device__-only overload in HIP's headers: a portable test for the code shared by the GPU and the host threads.)
// A comparison, not `v - v == 0`: the device compiler contracts across statements, and with v = a * w still in a register it turned
// v - v into fma(a, w, -v), the product's rounding error -- nonzero unless w is 1, so bd_solve_pnp failed EVERY pose with fx != fy
// (tests/test_gpu_pnp_regimes.py, regime `aniso`; the host build and the wave form, which reads v back from LDS, never did).
__host__ __device__ inline bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }

// cyclic Jacobi eigen-decomposition of a symmetric n x n matrix (row-major, destroyed); V columns = eigenvectors
template <int N> __host__ __device__ void jacobi_eig(double* A, double* V, double* w) {
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) V[i * N + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < N; ++i) {
            diag += A[i * N + i] * A[i * N + i];
            for (int j = i + 1; j < N; ++j) off += A[i * N + j] * A[i * N + j];
        }
        if (off <= 1e-60 || off <= 1e-32 * diag) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p * N + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * N + q] - A[p * N + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < N; ++k) {
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    A[k * N + p] = c * akp - s * akq;
                    A[k * N + q] = s * akp + c * akq;
                }
                for (int k = 0; k < N; ++k) {
                    const double apk = A[p * N + k], aqk = A[q * N + k];
                    A[p * N + k] = c * apk - s * aqk;
                    A[q * N + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < N; ++k) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < N; ++i) w[i] = A[i * N + i];
}

__host__ __device__ double det3(const double* R) {
    return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

__host__ __device__ void rodrigues(const double* rv, double* R) {
    const double th = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    if (th < 1e-12) {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double k0 = rv[0] / th, k1 = rv[1] / th, k2 = rv[2] / th, s = sin(th), c1 = 1.0 - cos(th);
    const double Kx[9] = {0, -k2, k1, k2, 0, -k0, -k1, k0, 0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0.0;
            for (int m = 0; m < 3; ++m) kk += Kx[i * 3 + m] * Kx[m * 3 + j];
            R[i * 3 + j] = (i == j ? 1.0 : 0.0) + s * Kx[i * 3 + j] + c1 * kk;
        }
}

// (no dynamic index, here and in solve6: in the wave kernels, which have no scratch, the arrays stay in registers)
__host__ __device__ inline void rvec_from_R(const double* R, double* rv) {
    double c = (R[0] + R[4] + R[8] - 1.0) / 2.0;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double th = acos(c);
    if (th < 1e-8) { rv[0] = rv[1] = rv[2] = 0.0; return; }
    if (3.14159265358979323846 - th < 1e-4) {            // near pi: dominant column of (R + I) / 2
        double A[9];
        for (int i = 0; i < 9; ++i) A[i] = (R[i] + (i % 4 == 0 ? 1.0 : 0.0)) / 2.0;
        int k = 0;
        double dk = A[0];
        if (A[4] > dk) { k = 1; dk = A[4]; }
        if (A[8] > dk) { k = 2; dk = A[8]; }
        const double d = sqrt(dk > 1e-12 ? dk : 1e-12);
        for (int i = 0; i < 3; ++i) rv[i] = (k == 0 ? A[i * 3] : (k == 1 ? A[i * 3 + 1] : A[i * 3 + 2])) / d * th;
        return;
    }
    const double f = th / (2.0 * sin(th));
    rv[0] = (R[7] - R[5]) * f; rv[1] = (R[2] - R[6]) * f; rv[2] = (R[3] - R[1]) * f;
}

// residuals of pose x = (rvec, t) for n points; returns false on a non-finite value.  OpenCV's ITERATIVE solver minimises the
// reprojection error in PIXELS, i.e. it weights the normalised x / y residuals by fx / fy: (wx, wy) = (fx, fy) / sqrt(fx fy) gives the
// same minimiser and is exactly (1, 1) for square pixels.
__host__ __device__ bool residuals(const double* x, const double* p3, const double* p2n, int n, double* r, double wx, double wy) {
    double R[9];
    rodrigues(x, R);
    bool ok = true;
    for (int i = 0; i < n; ++i) {
        const double X = p3[i * 3], Y = p3[i * 3 + 1], Z = p3[i * 3 + 2];
        const double cx = R[0] * X + R[1] * Y + R[2] * Z + x[3], cy = R[3] * X + R[4] * Y + R[5] * Z + x[4],
                     cz = R[6] * X + R[7] * Y + R[8] * Z + x[5];
        r[2 * i] = (cx / cz - p2n[2 * i]) * wx;
        r[2 * i + 1] = (cy / cz - p2n[2 * i + 1]) * wy;
        ok = ok && finite_d(r[2 * i]) && finite_d(r[2 * i + 1]);
    }
    return ok;
}

// solve the 6 x 6 system H d = g (partial pivoting; the pivot row is swapped in through selects); false if singular
__host__ __device__ inline bool solve6(double (&H)[36], double (&g)[6], double (&d)[6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        double best = fabs(H[c * 6 + c]);
#pragma unroll
        for (int r = c + 1; r < 6; ++r) if (fabs(H[r * 6 + c]) > best) { piv = r; best = fabs(H[r * 6 + c]); }
        if (best < 1e-300) return false;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int k = 0; k < 6; ++k) { const double a = H[c * 6 + k], b = H[r * 6 + k]; H[c * 6 + k] = sw ? b : a; H[r * 6 + k] = sw ? a : b; }
            const double a = g[c], b = g[r]; g[c] = sw ? b : a; g[r] = sw ? a : b;
        }
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            const double f = H[r * 6 + c] / H[c * 6 + c];
#pragma unroll
            for (int k = c; k < 6; ++k) H[r * 6 + k] -= f * H[c * 6 + k];
            g[r] -= f * g[c];
        }
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = g[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) s -= H[r * 6 + k] * d[k];
        d[r] = s / H[r * 6 + r];
    }
    return true;
}

// The stop rule of every form.  pred = d . (g + lam D d) is the decrease of the squared error that the linearisation promises for the
// damped step d (lam D d = g - H d, so this is 2 d.g - d^T H d); e0 the squared error at x, both in normalised image coordinates
// (dimensionless: neither the model's unit nor the intrinsics enter).  Where the promise falls below 1e-12 of the error the step is
// not taken.  Under weak damping (lam <= 1e-3) that is convergence: the Gauss-Newton decrease exceeds the damped one by at most
// ~lam / (2 mu), mu the eigenvalue of the scaled J^T J, far below the 1e-6 the tests allow.  Under strong damping it only says the
// step is short: lam goes back to 1e-3 and the iteration goes on.  The absolute floor is for exact corners: there e0 is only the fp32
// rounding of the pixels (~1e-16), the promise of a step stays at ~1e-9 e0 (the forward differences see that rounding, not a slope)
// while no step lowers the error, and without a floor the solve cycles to its cap.  1e-20 is a squared residual of 1e-10 in
// normalised coordinates: 6e-8 px at f = 600, a few thousandths of the spacing of the fp32 pixels the solver is given.
__host__ __device__ inline bool lm_converged(double pred, double e0) { return pred <= 1e-12 * e0 + 1e-20; }

// What `iters` means.  From LM_STRICT_ITERS on it is a CAP for a caller who wants the minimum (the callers pass 400): a well-posed
// pose stops after about ten iterations, a hard one runs until it is stationary, and a solve that leaves the loop any other way -- the
// cap, or a singular system -- has NO pose (zeros, rms 0, the RANSAC's fall-back), like a point behind the camera: a caller is never
// handed an iterate from a slope as a solved pose.  Below it `iters` is a BUDGET, and the iterate is returned as it stands: the
// RANSAC's hypotheses (5 iterations, scored and then discarded) and the DLT start alone (0).
constexpr int LM_STRICT_ITERS = 100;
__host__ __device__ inline bool lm_unfinished(bool converged, int iters) { return !converged && iters >= LM_STRICT_ITERS; }

// The Levenberg-Marquardt rule of every form, once.  A driver owns the loop over `iters` and how the sums are produced -- serial loops
// in the thread form, phases over the lanes in the wave form: per iteration H = J^T J, g = -J^T r and e0 = |r|^2 at L.x go to
// lm_propose; where that answers LM_TRY the driver evaluates e1 = |r|^2 at L.xn and lm_accept takes or rejects the step; after the
// loop lm_finish says whether there is a pose.  Every decision goes through run.uniform() where it is taken: in the wave form that makes
// it a scalar branch (decided on lane values it cost 2 % of a launch that runs to the cap); the thread form passes OneLane.
struct LmState {
    double x[6], xn[6];               // the iterate (rvec, t) and the candidate of the last lm_propose
    double lam = 1e-3;
    bool converged = false;
};
enum LmNext { LM_TRY, LM_AGAIN, LM_STOP };      // evaluate L.xn; go round again at the same x; leave the loop
struct OneLane { __host__ __device__ bool uniform(bool b) const { return b; } };      // the thread form's `run`: a pose is one lane's

// H and g are destroyed.  The damping scales with the diagonal (floored at 1e-12, so a zero column of J is damped too).
template <class Run> __host__ __device__ inline LmNext lm_propose(const Run& run, LmState& L, double (&H)[36], double (&g)[6], double e0) {
    double g0[6], D[6], step[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) { g0[a] = g[a]; D[a] = H[a * 6 + a] + 1e-12; H[a * 6 + a] += L.lam * D[a]; }
    if (!run.uniform(solve6(H, g, step))) return LM_STOP;                  // singular: not converged
    double pred = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) { L.xn[k] = L.x[k] + step[k]; pred += step[k] * (g0[k] + L.lam * D[k] * step[k]); }
    if (!run.uniform(lm_converged(pred, e0))) return LM_TRY;
    if (L.lam <= 1e-3) { L.converged = true; return LM_STOP; }
    L.lam = 1e-3;
    return LM_AGAIN;
}

// (a non-finite residual at xn makes e1 inf or NaN, and the step is rejected)
template <class Run> __host__ __device__ inline bool lm_accept(const Run& run, LmState& L, double e0, double e1) {
    if (!run.uniform(e1 < e0)) { L.lam *= 10.0; return false; }
#pragma unroll
    for (int k = 0; k < 6; ++k) L.x[k] = L.xn[k];
    L.lam = L.lam * 0.3 > 1e-9 ? L.lam * 0.3 : 1e-9;
    return true;
}

// R = the rotation of L.x.  False: no pose -- a minimum was asked for and not reached (lm_unfinished), or a point lies at or behind the
// camera plane (zeros, like a NaN corner).  pts: point i at pts[i * stride .. + 2].
template <class Run> __host__ __device__ inline bool lm_finish(const Run& run, const LmState& L, int iters, const double* pts, int stride, int n, double (&R)[9]) {
    if (run.uniform(lm_unfinished(L.converged, iters))) return false;
    rodrigues(L.x, R);
    bool front = true;
    for (int i = 0; i < n; ++i) {                              // (no early exit: the loads of a wave's 64 points overlap)
        const double z = R[6] * pts[i * stride] + R[7] * pts[i * stride + 1] + R[8] * pts[i * stride + 2] + L.x[5];
        front = front && z > 0.0;
    }
    return run.uniform(front);
}

// The DLT start's translation t, given d = max over the points of -(R p)_z: the nearest point lies at depth t_z - d.  Where that is not
// positive, t is stretched along its own direction (the box centre keeps its pixel) to t_z = 2 d; a t_z <= 0 is replaced by 2 d.
__host__ __device__ inline void depth_clear(double* t, double d) {
    if (!(d > 0.0) || t[2] > d) return;
    if (t[2] > 0.0) { const double s = 2.0 * d / t[2]; t[0] *= s; t[1] *= s; t[2] *= s; }
    else t[2] = 2.0 * d;
}

// The DLT start of every form: x = (rvec, t) from the null vector P (3 x 4, row-major) of the DLT system, the points' mean and the
// points (point i at pts[i * stride .. + 2]); false where P[:, :3] has no rank 3.  Every index is static but the one over the points.
__host__ __device__ inline bool dlt_start(const double (&P)[12], const double (&mean)[3], const double* pts, int stride, int n, double (&x)[6]) {
    // ---- nearest rotation to M = P[:, :3]: M = U S V^T, R = U V^T (through the eigen-decomposition of M^T M)
    double M[9], MtM[9], V[9], s2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i * 3 + j] = P[i * 4 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += M[k * 3 + i] * M[k * 3 + j];
            MtM[i * 3 + j] = s;
        }
    jacobi_eig<3>(MtM, V, s2);
    auto order = [&](int a, int b) {                           // descending singular values (numpy's order), as compare-and-swaps
        if (s2[b] > s2[a]) {
            const double t = s2[a]; s2[a] = s2[b]; s2[b] = t;
#pragma unroll
            for (int i = 0; i < 3; ++i) { const double u = V[i * 3 + a]; V[i * 3 + a] = V[i * 3 + b]; V[i * 3 + b] = u; }
        }
    };
    order(0, 1); order(0, 2); order(1, 2);
    double sig[3], U[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) sig[c] = sqrt(s2[c] > 0 ? s2[c] : 0.0);
    if (!(sig[2] > 0.0)) return false;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += M[i * 3 + k] * V[k * 3 + c];
            U[i * 3 + c] = s / sig[c];
        }
    double R[9], t[3];
    auto UVt = [&]() {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) s += U[i * 3 + c] * V[j * 3 + c];
                R[i * 3 + j] = s;
            }
    };
    auto negate_R = [&]() {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = -R[i];
    };
    UVt();
    // ---- sign fixes
    double scale = (sig[0] + sig[1] + sig[2]) / 3.0;
    if (det3(R) < 0) { negate_R(); scale = -scale; }
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = P[i * 4 + 3] / scale;
    const double zc = R[6] * mean[0] + R[7] * mean[1] + R[8] * mean[2] + t[2];
    if (zc < 0) {                                              // points must be in front of the camera
        negate_R();
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = -t[i];
        // -R is improper: the nearest PROPER rotation to the negated M is -(U' V^T), U' = U with its last column negated, where
        // det(U V^T) was +1, and U' V^T where it was -1 (the sign of the null vector P, which the eigen-solver is free to choose)
        if (det3(R) < 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) U[i * 3 + 2] = -U[i * 3 + 2];
            UVt();
            if (det3(R) < 0) negate_R();
        }
    }
    {   // a start with a point at or behind the camera plane (noisy corners of a far or flat box) sits in the basin of a mirrored pose
        // that LM cannot leave: move it out along its own viewing ray until the nearest point is as deep as the model is (depth_clear)
        double d = -1e300;
        for (int i = 0; i < n; ++i) {
            const double q = -(R[6] * pts[i * stride] + R[7] * pts[i * stride + 1] + R[8] * pts[i * stride + 2]);
            d = q > d ? q : d;
        }
        depth_clear(t, d);
    }
    rvec_from_R(R, x);
    x[3] = t[0]; x[4] = t[1]; x[5] = t[2];
    return true;
}

// One pose: kp [n, 2] pixels, pts3 [n, 3], Kp [3, 3] -> out [4, 4] = [R|t; 0 0 0 1], all zeros where the solve fails.  The same code
// runs per GPU thread (pnp_kernel) and per host worker thread (bd_solve_pnp_host).
__host__ __device__ void solve_one_pose(const float* kp, const float* pts3, const float* Kp, int n, int iters, float* out) {
    for (int i = 0; i < 16; ++i) out[i] = 0.f;
    double p3[MAXPTS * 3], p2n[MAXPTS * 2];
    const double fx = Kp[0], fy = Kp[4], cx = Kp[2], cy = Kp[5];
    double mean[3] = {0, 0, 0};
    bool ok = true;
    for (int i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) { p3[i * 3 + c] = pts3[i * 3 + c]; mean[c] += p3[i * 3 + c] / n; }
        p2n[2 * i] = ((double)kp[i * 2] - cx) / fx;
        p2n[2 * i + 1] = ((double)kp[i * 2 + 1] - cy) / fy;
        ok = ok && finite_d(p2n[2 * i]) && finite_d(p2n[2 * i + 1]);
    }
    if (!ok) return;
    // ---- DLT: null vector of A (2n x 12) = eigenvector of A^T A with the smallest eigenvalue
    double AtA[144], V[144], w[12];
    for (int i = 0; i < 144; ++i) AtA[i] = 0.0;
    for (int i = 0; i < n; ++i) {
        const double X[4] = {p3[i * 3], p3[i * 3 + 1], p3[i * 3 + 2], 1.0};
        double r1[12], r2[12];
        for (int c = 0; c < 4; ++c) {
            r1[c] = X[c]; r1[4 + c] = 0.0; r1[8 + c] = -p2n[2 * i] * X[c];
            r2[c] = 0.0; r2[4 + c] = X[c]; r2[8 + c] = -p2n[2 * i + 1] * X[c];
        }
        for (int a = 0; a < 12; ++a)
            for (int b = 0; b < 12; ++b) AtA[a * 12 + b] += r1[a] * r1[b] + r2[a] * r2[b];
    }
    jacobi_eig<12>(AtA, V, w);
    int kmin = 0;
    for (int i = 1; i < 12; ++i) if (w[i] < w[kmin]) kmin = i;
    double P[12];
    for (int i = 0; i < 12; ++i) P[i] = V[i * 12 + kmin];
    LmState L;
    if (!dlt_start(P, mean, p3, 3, n, L.x)) return;
    // ---- Levenberg-Marquardt on (rvec, t): J, J^T J, g and the errors in serial loops, all of them again in every iteration
    double r[MAXPTS * 2], rn[MAXPTS * 2], J[MAXPTS * 2 * 6];
    const double fgm = sqrt(fabs(fx * fy)), wx = fgm > 0 ? fabs(fx) / fgm : 1.0, wy = fgm > 0 ? fabs(fy) / fgm : 1.0;
    if (!residuals(L.x, p3, p2n, n, r, wx, wy)) return;
    const int m = 2 * n;
    for (int it = 0; it < iters; ++it) {
        for (int j = 0; j < 6; ++j) {
            double xd[6];
            for (int k = 0; k < 6; ++k) xd[k] = L.x[k];
            xd[j] += 1e-6;
            residuals(xd, p3, p2n, n, rn, wx, wy);
            for (int i = 0; i < m; ++i) {
                const double d = (rn[i] - r[i]) / 1e-6;
                J[i * 6 + j] = finite_d(d) ? d : 0.0;
            }
        }
        double H[36], g[6], e0 = 0.0, e1 = 0.0;
        for (int a = 0; a < 6; ++a) {
            double s = 0.0;
            for (int i = 0; i < m; ++i) s += J[i * 6 + a] * r[i];
            g[a] = -s;
            for (int b = 0; b < 6; ++b) {
                double h = 0.0;
                for (int i = 0; i < m; ++i) h += J[i * 6 + a] * J[i * 6 + b];
                H[a * 6 + b] = h;
            }
        }
        for (int i = 0; i < m; ++i) e0 += r[i] * r[i];
        const LmNext next = lm_propose(OneLane(), L, H, g, e0);
        if (next == LM_STOP) break;
        if (next == LM_AGAIN) continue;
        residuals(L.xn, p3, p2n, n, rn, wx, wy);
        for (int i = 0; i < m; ++i) e1 += rn[i] * rn[i];
        if (lm_accept(OneLane(), L, e0, e1))
            for (int i = 0; i < m; ++i) r[i] = rn[i];
    }
    double R[9];
    if (!lm_finish(OneLane(), L, iters, p3, 3, n, R)) return;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out[i * 4 + j] = (float)R[i * 3 + j];
        out[i * 4 + 3] = (float)L.x[3 + i];
    }
    out[15] = 1.f;
}

__global__ __launch_bounds__(64) void pnp_kernel(const float* __restrict__ kp, const float* __restrict__ pts3,
                                                 const float* __restrict__ Kmat, int N, int n, int iters,
                                                 float* __restrict__ poses) {
    const int id = blockIdx.x * 64 + threadIdx.x;
    if (id >= N) return;
    solve_one_pose(kp + (size_t)id * n * 2, pts3 + (size_t)id * n * 3, Kmat + (size_t)id * 9, n, iters, poses + (size_t)id * 16);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The wave form: ONE wavefront (64 lanes) per pose, solve_one_pose's algorithm in fp64 around the same dlt_start and LM rule.  The solver is written as a
// DRIVER (pnp_wave_solve) around PHASES.  A phase is a function of (lane, shared state): it reads what earlier phases left in the
// shared state and writes locations no other lane of the same phase reads; `run(phase)` executes it on all 64 lanes between two
// barriers.  Driver code between the phases is executed by every lane on the same shared values in the same order, so every lane holds
// the same bits; the values that decide a branch or a loop exit go through run.uniform() (v_readfirstlane) on top of that.  Nothing is
// indexed dynamically outside the shared state (LDS): the kernel has no scratch.  Every sum runs in index order without atomics, and a
// workgroup is one pose, so a pose's bits do not depend on the batch.  On the host the same driver runs with a runner that loops over
// the 64 lanes (LoopRun; tools/pnp_wave_hostcheck.cpp: the index arithmetic under the address / undefined-behaviour sanitizers, no GPU).
struct WaveState {
    double p4[MAXPTS * 4];            // (X, Y, Z, 1) per point
    double p2n[MAXPTS * 2];           // normalised image coordinates
    double A[2][144], V[2][144];      // Jacobi: read one copy, write the other
    double cs[24];                    // per index i of the current Jacobi step: cc[i], ss[i]
    double Rt[6][12];                 // [R | t] of the six perturbed poses
    double r[2][MAXPTS * 2];          // residuals at x / at the candidate (the roles swap on an accepted step)
    double J[MAXPTS * 2 * 6];
    double Hg[27];                    // J^T J (21 distinct entries, upper triangle by rows), then g (6)
    float out[16];
};

// partner of index i in step r (0..10) of the round-robin ordering of 12 indices: 6 disjoint pairs per step, every pair once per sweep
__host__ __device__ inline int rr_partner(int i, int r) {
    if (i == 11) return r;
    if (i == r) return 11;
    const int p = 2 * r - i;
    return p < 0 ? p + 11 : (p >= 11 ? p - 11 : p);
}
// e-th entry (row-major) of the upper triangle, diagonal included, of an N x N matrix
template <int N> __host__ __device__ inline void tri_entry(int e, int& i, int& j) {
    i = 0;
    for (int k = 0; k < N - 1; ++k)
        if (e >= N - i) { e -= N - i; ++i; }
    j = i + e;
}

// One pose by one "wave" of 64 lanes.  Returns false where solve_one_pose leaves zeros; on success S.out holds the 4 x 4 pose and
// *rms_out the root mean square of the PIXEL reprojection error of that pose (of its fp32 rounding, which is what the caller gets).  `run(f)` executes f(lane) for lane = 0 .. 63 with a
// barrier before and after; `run.uniform(b)` returns b, the same in every lane.  Rt64 (may be null): 12 doubles of the caller's, every
// lane's own copy: the pose BEFORE its rounding to fp32, R row-major then t (the RANSAC scores its hypotheses with it).
template <class Run>
__host__ __device__ inline bool pnp_wave_solve(const Run& run, WaveState& S, const float* kp, const float* pts3, const float* Kp, int n,
                                               int iters, double* rms_out, double* Rt64 = nullptr) {
    const double fx = Kp[0], fy = Kp[4], cx = Kp[2], cy = Kp[5];
    const int m = 2 * n;
    // ---- 1. normalise: lane = point
    run([&](int lane) {
        if (lane >= n) return;
        for (int c = 0; c < 3; ++c) S.p4[lane * 4 + c] = pts3[lane * 3 + c];
        S.p4[lane * 4 + 3] = 1.0;
        S.p2n[2 * lane] = ((double)kp[lane * 2] - cx) / fx;
        S.p2n[2 * lane + 1] = ((double)kp[lane * 2 + 1] - cy) / fy;
    });
    bool ok = true;
    double mean[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) mean[c] += S.p4[i * 4 + c] / n;
        ok = ok && finite_d(S.p2n[2 * i]) && finite_d(S.p2n[2 * i + 1]);
    }
    if (!run.uniform(ok)) return false;
    // ---- 2. DLT: A^T A, a lane owns entries lane, lane + 64, lane + 128 and sums over the points in index order; V = I
    run([&](int lane) {
        for (int e = lane; e < 144; e += 64) {
            const int a = e / 12, b = e % 12, ba = a / 4, bb = b / 4, ca = a % 4, cb = b % 4;
            double s = 0.0;
            for (int i = 0; i < n; ++i) {
                const double Xa = S.p4[i * 4 + ca], Xb = S.p4[i * 4 + cb], u = S.p2n[2 * i], v = S.p2n[2 * i + 1];
                const double r1a = ba == 0 ? Xa : (ba == 2 ? -u * Xa : 0.0), r1b = bb == 0 ? Xb : (bb == 2 ? -u * Xb : 0.0);
                const double r2a = ba == 1 ? Xa : (ba == 2 ? -v * Xa : 0.0), r2b = bb == 1 ? Xb : (bb == 2 ? -v * Xb : 0.0);
                s += r1a * r1b + r2a * r2b;
            }
            S.A[0][e] = s;
            S.V[0][e] = a == b ? 1.0 : 0.0;
        }
    });
    // ---- Jacobi on the 12 x 12: round-robin ordering, the 6 disjoint rotations of a step applied at once (A <- J^T A J, V <- V J)
    int cur = 0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 12; ++i) {
            diag += S.A[cur][i * 12 + i] * S.A[cur][i * 12 + i];
            for (int j = i + 1; j < 12; ++j) off += S.A[cur][i * 12 + j] * S.A[cur][i * 12 + j];
        }
        if (run.uniform(off <= 1e-60 || off <= 1e-32 * diag)) break;
        for (int step = 0; step < 11; ++step) {
            run([&](int lane) {                       // rotation of the pair that index `lane` belongs to
                if (lane >= 12) return;
                const int ip = rr_partner(lane, step), p = lane < ip ? lane : ip, q = lane < ip ? ip : lane;
                const double apq = S.A[cur][p * 12 + q];
                double c = 1.0, s = 0.0;
                if (apq != 0.0) {
                    const double theta = (S.A[cur][q * 12 + q] - S.A[cur][p * 12 + p]) / (2.0 * apq);
                    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                }
                S.cs[2 * lane] = c;
                S.cs[2 * lane + 1] = lane == p ? -s : s;
            });
            run([&](int lane) {
                for (int e = lane; e < 78; e += 64) {            // A: upper triangle, mirrored
                    int i, j;
                    tri_entry<12>(e, i, j);
                    const int ip = rr_partner(i, step), jp = rr_partner(j, step);
                    const double ci = S.cs[2 * i], si = S.cs[2 * i + 1], cj = S.cs[2 * j], sj = S.cs[2 * j + 1];
                    const double* A = S.A[cur];
                    const double v = ci * (cj * A[i * 12 + j] + sj * A[i * 12 + jp]) + si * (cj * A[ip * 12 + j] + sj * A[ip * 12 + jp]);
                    S.A[cur ^ 1][i * 12 + j] = v;
                    S.A[cur ^ 1][j * 12 + i] = v;
                }
                for (int e = lane; e < 144; e += 64) {
                    const int k = e / 12, j = e % 12, jp = rr_partner(j, step);
                    S.V[cur ^ 1][e] = S.cs[2 * j] * S.V[cur][e] + S.cs[2 * j + 1] * S.V[cur][k * 12 + jp];
                }
            });
            cur ^= 1;
        }
    }
    int kmin = 0;
    double wmin = S.A[cur][0];
    for (int i = 1; i < 12; ++i) { const double w = S.A[cur][i * 12 + i]; if (w < wmin) { wmin = w; kmin = i; } }
    double P[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = S.V[cur][i * 12 + kmin];
    // ---- 3. / 4. the DLT start (every lane, in registers)
    LmState L;
    if (!run.uniform(dlt_start(P, mean, S.p4, 4, n, L.x))) return false;
    // ---- 5. / 6. Levenberg-Marquardt on (rvec, t): J, J^T J and g in phases over the lanes, kept while x stays; e0 carried along
    double R[9];
    const double fgm = sqrt(fabs(fx * fy)), wx = fgm > 0 ? fabs(fx) / fgm : 1.0, wy = fgm > 0 ? fabs(fy) / fgm : 1.0;
    int rb = 0;
    double tr[3];
    auto residuals_into = [&](int buf) {                       // lane = point: residuals of the pose (R, tr) into S.r[buf]
        run([&](int lane) {
            if (lane >= n) return;
            const double X = S.p4[lane * 4], Y = S.p4[lane * 4 + 1], Z = S.p4[lane * 4 + 2];
            const double pcx = R[0] * X + R[1] * Y + R[2] * Z + tr[0], pcy = R[3] * X + R[4] * Y + R[5] * Z + tr[1],
                         pcz = R[6] * X + R[7] * Y + R[8] * Z + tr[2];
            S.r[buf][2 * lane] = (pcx / pcz - S.p2n[2 * lane]) * wx;
            S.r[buf][2 * lane + 1] = (pcy / pcz - S.p2n[2 * lane + 1]) * wy;
        });
    };
    rodrigues(L.x, R);
    tr[0] = L.x[3]; tr[1] = L.x[4]; tr[2] = L.x[5];
    residuals_into(rb);
    double e0 = 0.0;
    bool fin = true;
    for (int i = 0; i < m; ++i) { const double v = S.r[rb][i]; fin = fin && finite_d(v); e0 += v * v; }
    if (!run.uniform(fin)) return false;
    bool fresh = true;                                         // x moved: J, J^T J and g are rebuilt (a rejected step keeps them)
    for (int it = 0; it < iters; ++it) {
        if (fresh) {
            run([&](int lane) {                                // lanes 0 .. 5: [R | t] of x + h e_lane
                double xd[6], Rd[9];
#pragma unroll
                for (int k = 0; k < 6; ++k) xd[k] = L.x[k] + (k == lane ? 1e-6 : 0.0);
                rodrigues(xd, Rd);
                if (lane >= 6) return;
#pragma unroll
                for (int k = 0; k < 9; ++k) S.Rt[lane][k] = Rd[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) S.Rt[lane][9 + k] = xd[3 + k];
            });
            run([&](int lane) {                                // 6 perturbations x n points over the lanes
                for (int w = lane; w < 6 * n; w += 64) {
                    const int j = w / n, i = w - j * n;
                    const double* Q = S.Rt[j];
                    const double X = S.p4[i * 4], Y = S.p4[i * 4 + 1], Z = S.p4[i * 4 + 2];
                    const double pcx = Q[0] * X + Q[1] * Y + Q[2] * Z + Q[9], pcy = Q[3] * X + Q[4] * Y + Q[5] * Z + Q[10],
                                 pcz = Q[6] * X + Q[7] * Y + Q[8] * Z + Q[11];
                    const double d0 = ((pcx / pcz - S.p2n[2 * i]) * wx - S.r[rb][2 * i]) / 1e-6;
                    const double d1 = ((pcy / pcz - S.p2n[2 * i + 1]) * wy - S.r[rb][2 * i + 1]) / 1e-6;
                    S.J[(2 * i) * 6 + j] = finite_d(d0) ? d0 : 0.0;
                    S.J[(2 * i + 1) * 6 + j] = finite_d(d1) ? d1 : 0.0;
                }
            });
            run([&](int lane) {                                // one lane per distinct entry of J^T J and of g, rows in index order
                if (lane < 21) {
                    int a, b;
                    tri_entry<6>(lane, a, b);
                    double h = 0.0;
                    for (int i = 0; i < m; ++i) h += S.J[i * 6 + a] * S.J[i * 6 + b];
                    S.Hg[lane] = h;
                } else if (lane < 27) {
                    const int a = lane - 21;
                    double s = 0.0;
                    for (int i = 0; i < m; ++i) s += S.J[i * 6 + a] * S.r[rb][i];
                    S.Hg[lane] = -s;
                }
            });
            fresh = false;
        }
        double H[36], g[6], e1 = 0.0;
        {
            int e = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b, ++e) { H[a * 6 + b] = S.Hg[e]; H[b * 6 + a] = S.Hg[e]; }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) g[a] = S.Hg[21 + a];
        const LmNext next = lm_propose(run, L, H, g, e0);
        if (next == LM_STOP) break;
        if (next == LM_AGAIN) continue;
        rodrigues(L.xn, R);
        tr[0] = L.xn[3]; tr[1] = L.xn[4]; tr[2] = L.xn[5];
        residuals_into(rb ^ 1);
        for (int i = 0; i < m; ++i) e1 += S.r[rb ^ 1][i] * S.r[rb ^ 1][i];
        if (lm_accept(run, L, e0, e1)) {
            rb ^= 1;
            e0 = e1;
            fresh = true;
        }
    }
    if (!lm_finish(run, L, iters, S.p4, 4, n, R)) return false;
    if (Rt64) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Rt64[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) Rt64[9 + i] = L.x[3 + i];
    }
    // ---- the pose, and its pixel reprojection error: lane = point, summed in index order
    run([&](int lane) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) S.out[i * 4 + j] = (float)R[i * 3 + j];
                S.out[i * 4 + 3] = (float)L.x[3 + i];
                S.out[12 + i] = 0.f;
            }
            S.out[15] = 1.f;
        }
        if (lane >= n) return;
        double Q[9], tq[3];                                    // the pose as it is returned: rounded to fp32
#pragma unroll
        for (int i = 0; i < 9; ++i) Q[i] = (double)(float)R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) tq[i] = (double)(float)L.x[3 + i];
        const double X = S.p4[lane * 4], Y = S.p4[lane * 4 + 1], Z = S.p4[lane * 4 + 2];
        const double pcx = Q[0] * X + Q[1] * Y + Q[2] * Z + tq[0], pcy = Q[3] * X + Q[4] * Y + Q[5] * Z + tq[1],
                     pcz = Q[6] * X + Q[7] * Y + Q[8] * Z + tq[2];
        const double du = (double)kp[lane * 2] - (fx * (pcx / pcz) + cx), dv = (double)kp[lane * 2 + 1] - (fy * (pcy / pcz) + cy);
        S.r[0][lane] = du * du + dv * dv;                      // (the residuals are no longer needed)
    });
    double ss = 0.0;
    for (int i = 0; i < n; ++i) ss += S.r[0][i];
    *rms_out = sqrt(ss / n);
    return true;
}

struct WaveRun {
    template <class F> __device__ __forceinline__ void operator()(F f) const {
        __syncthreads();                        // one wave per workgroup: the wait for its own LDS traffic, and a fence
        f((int)threadIdx.x);
        __syncthreads();
    }
    __device__ __forceinline__ bool uniform(bool b) const { return __builtin_amdgcn_readfirstlane((int)b) != 0; }
};

// grid = n_poses, ONE wave per workgroup: a wave that shared a barrier with the waves of other poses could wait for ever on a pose
// that needs fewer sweeps or LM iterations
__global__ __launch_bounds__(64) void pnp_wave_kernel(const float* __restrict__ kp, const float* __restrict__ pts3,
                                                      const float* __restrict__ Kmat, int n, int iters, float* __restrict__ poses,
                                                      float* __restrict__ rms_px) {
    __shared__ WaveState S;
    const size_t id = blockIdx.x;
    const int lane = threadIdx.x;
    double rms = 0.0;
    const bool ok = pnp_wave_solve(WaveRun(), S, kp + id * n * 2, pts3 + id * n * 3, Kmat + id * 9, n, iters, &rms);
    if (lane < 16) poses[id * 16 + lane] = ok ? S.out[lane] : 0.f;
    if (rms_px && lane == 0) rms_px[id] = ok ? (float)rms : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// RANSAC over the R x 8 corners of the dense multi-round mode (boxdreamer_amd/pnp.py: solve_pnp_ransac with a `picks` table), as two
// stages around pnp_wave_solve.  Stage 1, one wave per (sample, trial): solve the trial's 6 picked observations, score every observation
// of the sample against that pose.  Stage 2, one wave per sample: replay the host form's selection over the stored scores, then the
// final solve on the chosen inliers.  Both are written against `run` like the solver itself, so the host runs the same code with a
// loop over the lanes (LoopRun: bd_solve_pnp_ransac_host, tools/pnp_ransac_hostcheck.cpp).  Observation i of a sample is round i / 8,
// corner i % 8.
struct RansacObs {                    // the observations handed to pnp_wave_solve: a trial's 6, or the compacted inliers
    float kp[MAXPTS * 2];
    float p3[MAXPTS * 3];
};
struct RansacScore {                  // one hypothesis in the workspace
    double err_sum;                   // sum of the inliers' pixel errors, in index order (+inf where the solve failed)
    unsigned long long mask;          // bit i = observation i is an inlier
    int32_t count;                    // inliers, -1 where the solve failed
    int32_t pad;
};

template <class Run>
__host__ __device__ inline void ransac_gather(const Run& run, RansacObs& G, const float* kp, const float* box, unsigned long long mask, int n_obs) {
    run([&](int lane) {               // compaction in index order: the slot of an observation is the number of kept ones before it
        if (lane >= n_obs || !((mask >> lane) & 1ull)) return;
        const int k = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        G.kp[2 * k] = kp[2 * lane];
        G.kp[2 * k + 1] = kp[2 * lane + 1];
        for (int c = 0; c < 3; ++c) G.p3[3 * k + c] = box[(lane % 8) * 3 + c];
    });
}

// Stage 1.  kp [n_obs, 2], box [8, 3], Kp [3, 3] of the sample; pick6: the trial's 6 observation indices (clamped into [0, n_obs)).
// margin (host only, may be null): running minimum of |error - thr| over the scored observations.
template <class Run>
__host__ __device__ inline void ransac_hypothesis(const Run& run, WaveState& S, RansacObs& G, const float* kp, const float* box, const float* Kp,
                                                  const int32_t* pick6, int n_obs, double thr, int iters, RansacScore* out, double* margin) {
    run([&](int lane) {
        if (lane >= 6) return;
        int i = pick6[lane];
        i = i < 0 ? 0 : (i >= n_obs ? n_obs - 1 : i);
        G.kp[2 * lane] = kp[2 * i];
        G.kp[2 * lane + 1] = kp[2 * i + 1];
        for (int c = 0; c < 3; ++c) G.p3[3 * lane + c] = box[(i % 8) * 3 + c];
    });
    double Rt[12], rms = 0.0;
    const bool ok = pnp_wave_solve(run, S, G.kp, G.p3, Kp, 6, iters, &rms, Rt);
    int count = -1;
    double tot = __builtin_inf();
    unsigned long long mask = 0;
    if (ok) {
        const double fx = Kp[0], fy = Kp[4], cx = Kp[2], cy = Kp[5];
        run([&](int lane) {           // lane = observation: pixel error of the fp64 pose; behind the camera is never an inlier
            if (lane >= n_obs) return;
            const float* b = box + (lane % 8) * 3;
            const double X = b[0], Y = b[1], Z = b[2];
            const double pcx = Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[9], pcy = Rt[3] * X + Rt[4] * Y + Rt[5] * Z + Rt[10],
                         pcz = Rt[6] * X + Rt[7] * Y + Rt[8] * Z + Rt[11];
            const double z = fabs(pcz) < 1e-12 ? 1e-12 : pcz;
            const double du = pcx / z * fx + cx - (double)kp[2 * lane], dv = pcy / z * fy + cy - (double)kp[2 * lane + 1];
            S.r[0][lane] = pcz > 0 ? sqrt(du * du + dv * dv) : __builtin_inf();
        });
        count = 0;
        tot = 0.0;
        for (int i = 0; i < n_obs; ++i) {
            const double e = S.r[0][i];
            if (e < thr) { ++count; tot += e; mask |= 1ull << i; }
            if (margin && fabs(e - thr) < *margin) *margin = fabs(e - thr);
        }
    }
    run([&](int lane) {
        if (lane != 0) return;
        out->err_sum = tot;
        out->mask = mask;
        out->count = count;
        out->pad = 0;
    });
}

// Stage 2.  sc: the sample's n_trials scores.  Outputs of the sample: pose [16], inl [n_obs], rms_px / info (may be null).
template <class Run>
__host__ __device__ inline void ransac_final(const Run& run, WaveState& S, RansacObs& G, const float* kp, const float* box, const float* Kp,
                                             const RansacScore* sc, int n_obs, int n_trials, double confidence, int iters, float* pose,
                                             unsigned char* inl, float* rms_px, int32_t* info) {
    // ---- the selection of solve_pnp_ransac, batch by batch (32 trials): S.J is free here, [0, 64) counts and [64, 128) error sums
    int best = -1, best_cnt = -1, trials = 0;
    double best_err = __builtin_inf(), need = (double)n_trials;
    const int n_batches = (n_trials + 31) / 32;
    for (int b = 0; b < n_batches; ++b) {
        const int h = n_trials - trials < 32 ? n_trials - trials : 32;
        run([&](int lane) {
            if (lane >= h) return;
            S.J[lane] = (double)sc[trials + lane].count;
            S.J[64 + lane] = sc[trials + lane].err_sum;
        });
        int bi = 0;
        for (int i = 1; i < h; ++i) if (S.J[i] > S.J[bi]) bi = i;             // highest count, ties: lowest index
        const int c = (int)S.J[bi];
        const double e = S.J[64 + bi];
        if (c > best_cnt || (c == best_cnt && e < best_err)) { best_cnt = c; best_err = e; best = trials + bi; }
        trials += h;
        const double w = (double)(best_cnt > 0 ? best_cnt : 0) / (double)n_obs;
        bool stop = w >= 1.0;
        if (!stop && w > 0.0) {                                               // trials for `confidence` at this inlier ratio
            const double miss = 1.0 - w * w * w * w * w * w;
            need = ceil(log(1.0 - confidence) / log(miss > 1e-300 ? miss : 1e-300));
        }
        stop = stop || !((double)trials < (need < (double)n_trials ? need : (double)n_trials));
        if (run.uniform(stop)) break;
    }
    // ---- inliers of the best hypothesis, or every observation
    const unsigned long long all = n_obs >= 64 ? ~0ull : (1ull << n_obs) - 1ull;
    unsigned long long mask = best >= 0 ? sc[best].mask & all : 0ull;
    run([&](int lane) {
        if (lane < n_obs) S.r[0][lane] = finite_d((double)kp[2 * lane]) && finite_d((double)kp[2 * lane + 1]) ? 0.0 : 1.0;
    });
    bool finite = true;
    for (int i = 0; i < n_obs; ++i) finite = finite && S.r[0][i] == 0.0;
    unsigned corners = 0;
    for (int r = 0; r < n_obs / 8; ++r) corners |= (unsigned)(mask >> (8 * r)) & 0xffu;
    int path = (best_cnt < 6 || __builtin_popcount(corners) < 6 || !finite) ? 1 : 0;
    path = run.uniform(path != 0) ? 1 : 0;
    if (path) mask = all;
    bool ok = false;
    double rms = 0.0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        ransac_gather(run, G, kp, box, mask, n_obs);
        ok = pnp_wave_solve(run, S, G.kp, G.p3, Kp, __builtin_popcountll(mask), iters, &rms);
        if (ok || path) break;
        path = 1;                                                             // the inliers' solve failed: every observation
        mask = all;
    }
    if (!ok) { path = 2; mask = 0; }
    run([&](int lane) {
        if (lane < 16) pose[lane] = ok ? S.out[lane] : 0.f;
        if (lane < n_obs) inl[lane] = (unsigned char)((mask >> lane) & 1ull);
        if (lane != 0) return;
        if (rms_px) *rms_px = ok ? (float)rms : 0.f;
        if (info) { info[0] = trials; info[1] = best; info[2] = __builtin_popcountll(mask); info[3] = path; }
    });
}

struct LoopRun {                      // the 64 lanes of a "wave" one after the other: the host form
    template <class F> void operator()(F f) const { for (int lane = 0; lane < 64; ++lane) f(lane); }
    bool uniform(bool b) const { return b; }
};

// grid = n_samples * n_trials workgroups of one wave; no atomics, no workgroup waits for another
__global__ __launch_bounds__(64) void pnp_ransac_hyp_kernel(const float* __restrict__ kp, const float* __restrict__ box,
                                                            const float* __restrict__ Kmat, const int32_t* __restrict__ picks, int n_obs,
                                                            int n_trials, double thr, int iters, RansacScore* __restrict__ ws) {
    __shared__ WaveState S;
    __shared__ RansacObs G;
    const size_t id = blockIdx.x, s = id / (size_t)n_trials, t = id % (size_t)n_trials;
    ransac_hypothesis(WaveRun(), S, G, kp + s * n_obs * 2, box + s * 24, Kmat + s * 9, picks + t * 6, n_obs, thr, iters, ws + id, nullptr);
}

// grid = n_samples workgroups of one wave
__global__ __launch_bounds__(64) void pnp_ransac_final_kernel(const float* __restrict__ kp, const float* __restrict__ box,
                                                              const float* __restrict__ Kmat, const RansacScore* __restrict__ ws, int n_obs,
                                                              int n_trials, double confidence, int iters, float* __restrict__ poses,
                                                              unsigned char* __restrict__ inliers, float* __restrict__ rms_px,
                                                              int32_t* __restrict__ info) {
    __shared__ WaveState S;
    __shared__ RansacObs G;
    const size_t s = blockIdx.x;
    ransac_final(WaveRun(), S, G, kp + s * n_obs * 2, box + s * 24, Kmat + s * 9, ws + s * (size_t)n_trials, n_obs, n_trials, confidence, iters,
                 poses + s * 16, inliers + s * n_obs, rms_px ? rms_px + s : nullptr, info ? info + s * 4 : nullptr);
}

}  // namespace

// Host worker threads of bd_solve_pnp_host, kept between calls (round 6: starting seven std::threads per call was ~0.25 ms of the 0.36 ms
// a batch of 32 poses took -- device idle time in a facade forward, profiles/r6_facade_gaps.txt).  Library-owned HOST state (no device state):
// up to 15 detached threads per process, parked on a condition variable; one call at a time uses them (a mutex serialises callers); a forked
// child finds the parent's pid in the pool and starts its own.  Never torn down.
namespace {
struct HostPool {
    std::mutex m;
    std::condition_variable wake, done;
    const std::function<void(int)>* job = nullptr;
    int threads = 0, nt = 0, gen = 0, pending = 0;
    pid_t pid = 0;
};
std::mutex g_pool_mu;
HostPool* g_pool = nullptr;

void host_pool_worker(HostPool* P, int t) {
    int seen = 0;
    for (;;) {
        std::unique_lock<std::mutex> lk(P->m);
        P->wake.wait(lk, [&] { return P->gen != seen; });
        seen = P->gen;
        const std::function<void(int)>* job = P->job;
        const bool mine = t < P->nt;
        lk.unlock();
        if (!mine) continue;
        (*job)(t);
        lk.lock();
        if (--P->pending == 0) P->done.notify_one();
    }
}

void host_pool_run(int nt, const std::function<void(int)>& job) {      // job(0) on the caller, job(1 .. nt-1) on the pool
    std::lock_guard<std::mutex> callers(g_pool_mu);
    if (!g_pool || g_pool->pid != getpid() || g_pool->threads < nt - 1) {
        HostPool* P = new HostPool();                                    // (an older / inherited pool is left behind, its threads parked or gone)
        P->pid = getpid();
        P->threads = nt - 1 > 15 ? nt - 1 : 15;
        for (int t = 1; t <= P->threads; ++t) std::thread(host_pool_worker, P, t).detach();
        g_pool = P;
    }
    HostPool* P = g_pool;
    {
        std::lock_guard<std::mutex> lk(P->m);
        P->job = &job;
        P->nt = nt;
        P->pending = nt - 1;
        ++P->gen;
    }
    P->wake.notify_all();
    job(0);
    std::unique_lock<std::mutex> lk(P->m);
    P->done.wait(lk, [&] { return P->pending == 0; });
    P->job = nullptr;
}
}  // namespace

// The host form ("PnP post-solve stays on the host CPU", north_star): the same per-pose solver on a pool of host threads, poses
// dealt out in contiguous chunks.  All pointers are HOST pointers.  Replaces the per-sample Python loop around cv2.solvePnP of
// src/models/utils/box_utils.py:139-199 when OpenCV is not importable (and the single-threaded numpy restatement of round 2:
// 9 ms per 32 poses).  n_threads <= 0: one thread per 4 poses, at most 16.
extern "C" int bd_solve_pnp_host(const float* kp_px, const float* pts3, const float* K, int n_poses, int n_points, int iters,
                                 float* poses, int n_threads) {
    if (!kp_px || !pts3 || !K || !poses) return BD_ERR_NULL;
    if (n_poses <= 0 || n_points < 6 || n_points > MAXPTS || iters < 0) return BD_ERR_SHAPE;
    int nt = n_threads > 0 ? n_threads : (n_poses + 3) / 4;
    nt = nt > 16 ? 16 : (nt > n_poses ? n_poses : nt);
    auto work = [=](int t) {
        const int lo = (int)((int64_t)n_poses * t / nt), hi = (int)((int64_t)n_poses * (t + 1) / nt);
        for (int i = lo; i < hi; ++i)
            solve_one_pose(kp_px + (size_t)i * n_points * 2, pts3 + (size_t)i * n_points * 3, K + (size_t)i * 9, n_points, iters,
                           poses + (size_t)i * 16);
    };
    if (nt <= 1) { work(0); return BD_OK; }
    host_pool_run(nt, work);
    return BD_OK;
}

extern "C" int bd_solve_pnp(const float* kp_px, const float* pts3, const float* K, int n_poses, int n_points, int iters,
                            float* poses, void* stream) {
    if (!kp_px || !pts3 || !K || !poses) return BD_ERR_NULL;
    if (n_poses <= 0 || n_points < 6 || n_points > MAXPTS || iters < 0) return BD_ERR_SHAPE;
    hipLaunchKernelGGL(pnp_kernel, dim3((n_poses + 63) / 64), dim3(64), 0, (hipStream_t)stream, kp_px, pts3, K, n_poses,
                       n_points, iters, poses);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

// The wave form: one wavefront and one workgroup per pose (pnp_wave_kernel).  rms_px (fp32 [n_poses], may be NULL): root mean square of the
// pixel reprojection error of the returned pose over its n_points points, 0 where the solve fails.
extern "C" int bd_solve_pnp_wave(const float* kp_px, const float* pts3, const float* K, int n_poses, int n_points, int iters,
                                 float* poses, float* rms_px, void* stream) {
    if (!kp_px || !pts3 || !K || !poses) return BD_ERR_NULL;
    if (n_poses <= 0 || n_points < 6 || n_points > MAXPTS || iters < 0) return BD_ERR_SHAPE;
    hipLaunchKernelGGL(pnp_wave_kernel, dim3(n_poses), dim3(64), 0, (hipStream_t)stream, kp_px, pts3, K, n_points, iters, poses, rms_px);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

// RANSAC PnP over the n_rounds x 8 corners of the dense multi-round mode (replaces the cv2.solvePnPRansac call and its per-sample
// loop, src/models/utils/box_utils.py:202-300): pnp_ransac_hyp_kernel scores n_samples x n_trials hypotheses into the workspace,
// pnp_ransac_final_kernel selects and solves per sample.
namespace {
int ransac_args(const void* kp, const void* box, const void* K, const void* picks, const void* poses, const void* inliers, int n_samples,
                int n_rounds, int n_trials, int hyp_iters, int final_iters) {
    if (!kp || !box || !K || !picks || !poses || !inliers) return BD_ERR_NULL;
    if (n_samples <= 0 || n_rounds < 1 || n_rounds * 8 > MAXPTS || n_trials <= 0 || hyp_iters < 0 || final_iters < 0) return BD_ERR_SHAPE;
    if ((int64_t)n_samples * n_trials > INT_MAX) return BD_ERR_SHAPE;
    return BD_OK;
}
}  // namespace

extern "C" size_t bd_solve_pnp_ransac_workspace_bytes(int n_samples, int n_trials) {
    if (n_samples <= 0 || n_trials <= 0) return 0;
    return (size_t)n_samples * (size_t)n_trials * sizeof(RansacScore);
}

extern "C" int bd_solve_pnp_ransac_wave(const float* kp_px, const float* bbox_3d, const float* K, const int32_t* picks, int n_samples,
                                        int n_rounds, int n_trials, float reproj_err, float confidence, int hyp_iters, int final_iters,
                                        float* poses, unsigned char* inliers, float* rms_px, int32_t* info, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    const int rc = ransac_args(kp_px, bbox_3d, K, picks, poses, inliers, n_samples, n_rounds, n_trials, hyp_iters, final_iters);
    if (rc != BD_OK) return rc;
    if (!workspace) return BD_ERR_NULL;
    if (workspace_bytes < bd_solve_pnp_ransac_workspace_bytes(n_samples, n_trials)) return BD_ERR_SHAPE;
    RansacScore* ws = (RansacScore*)workspace;
    hipLaunchKernelGGL(pnp_ransac_hyp_kernel, dim3(n_samples * n_trials), dim3(64), 0, (hipStream_t)stream, kp_px, bbox_3d, K, picks,
                       n_rounds * 8, n_trials, (double)reproj_err, hyp_iters, ws);
    BD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pnp_ransac_final_kernel, dim3(n_samples), dim3(64), 0, (hipStream_t)stream, kp_px, bbox_3d, K,
                       (const RansacScore*)ws, n_rounds * 8, n_trials, (double)confidence, final_iters, poses, inliers, rms_px, info);
    BD_CHECK_LAUNCH();
    return BD_OK;
}

// The same two stages on the HOST through the loop runner (all pointers are host pointers): the hypotheses, then the samples, dealt out
// in contiguous chunks to the worker pool of bd_solve_pnp_host.  n_threads <= 0: at most 16.
extern "C" int bd_solve_pnp_ransac_host(const float* kp_px, const float* bbox_3d, const float* K, const int32_t* picks, int n_samples,
                                        int n_rounds, int n_trials, float reproj_err, float confidence, int hyp_iters, int final_iters,
                                        float* poses, unsigned char* inliers, float* rms_px, int32_t* info, int n_threads) {
    const int rc = ransac_args(kp_px, bbox_3d, K, picks, poses, inliers, n_samples, n_rounds, n_trials, hyp_iters, final_iters);
    if (rc != BD_OK) return rc;
    const int n_obs = n_rounds * 8, total = n_samples * n_trials;
    std::vector<RansacScore> ws((size_t)total);
    RansacScore* wsp = ws.data();
    int nt = n_threads > 0 ? n_threads : 16;
    nt = nt > 16 ? 16 : nt;
    auto stage = [&](int items, const std::function<void(int, WaveState&, RansacObs&)>& item) {
        const int n = nt > items ? items : nt;
        auto work = [&, n](int t) {
            std::unique_ptr<WaveState> S(new WaveState());
            std::unique_ptr<RansacObs> G(new RansacObs());
            const int lo = (int)((int64_t)items * t / n), hi = (int)((int64_t)items * (t + 1) / n);
            for (int i = lo; i < hi; ++i) item(i, *S, *G);
        };
        if (n <= 1) work(0); else host_pool_run(n, work);
    };
    stage(total, [&](int id, WaveState& S, RansacObs& G) {
        const size_t s = (size_t)(id / n_trials), t = (size_t)(id % n_trials);
        ransac_hypothesis(LoopRun(), S, G, kp_px + s * n_obs * 2, bbox_3d + s * 24, K + s * 9, picks + t * 6, n_obs, (double)reproj_err,
                          hyp_iters, wsp + id, nullptr);
    });
    stage(n_samples, [&](int i, WaveState& S, RansacObs& G) {
        const size_t s = (size_t)i;
        ransac_final(LoopRun(), S, G, kp_px + s * n_obs * 2, bbox_3d + s * 24, K + s * 9, wsp + s * (size_t)n_trials, n_obs, n_trials,
                     (double)confidence, final_iters, poses + s * 16, inliers + s * n_obs, rms_px ? rms_px + s : nullptr,
                     info ? info + s * 4 : nullptr);
    });
    return BD_OK;
}
