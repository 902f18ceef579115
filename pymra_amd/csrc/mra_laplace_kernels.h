// mra_laplace_kernels.h - kernels of mra_plan_fit_laplace and mra_plan_fit_laplace_trend (section 21): what runs
// between two Gaussian passes of the Newton iteration of a Laplace approximation.  Included by mra_launch_laplace.hip only, so that the
// other translation units keep their object code.
//
// Everything is by padded row.  A row is observed when its z is finite: the host uploads NaN at every row the plan does not observe.
// eta = x + offset; g = d log p / d eta; D = max(-d2 log p / d eta2, 2^-40).
#pragma once
#include "mra_plan_types.h"

static const int LAPLACE_BLOCKS = 1024;     // partial results of the reduction: a fixed number, folded in a fixed order (four workgroups per CU on 256 CUs)
static const int LAPLACE_NRES = 5;          // step, max |x^|, sum log D, sum D (t - x^)^2, sum of the x-dependent part of log p(z | eta^)

struct LaplaceTerm { double g, D, logp; };

// max(a, b) over values >= 0 that keeps a NaN from either side (fmax drops it): a NaN step must reach the host, which stops on it
__device__ __forceinline__ double laplace_max(double a, double b) { return (b > a || b != b) ? b : a; }

// g, D (floored) and the part of log p(z | eta) that depends on eta.  Gaussian: -(z - eta)^2 / (2 aux); Poisson: z eta - e^eta;
// binomial: z eta - aux log(1 + e^eta), with p and 1 - p from e^-|eta| so that neither saturates.
__device__ __forceinline__ LaplaceTerm laplace_term(int family, double z, double aux, double eta) {
    LaplaceTerm T;
    if (family == MRA_FAMILY_POISSON) {
        const double mu = exp(eta);
        T.g = z - mu; T.D = mu; T.logp = z * eta - mu;
    } else if (family == MRA_FAMILY_BINOMIAL) {
        const double e = exp(-fabs(eta)), s = 1.0 / (1.0 + e);
        const double p = eta >= 0.0 ? s : e * s, q = eta >= 0.0 ? e * s : s;
        T.g = z - aux * p; T.D = aux * p * q; T.logp = z * eta - aux * (fmax(eta, 0.0) + log1p(e));
    } else {
        const double res = z - eta;
        T.g = res / aux; T.D = 1.0 / aux; T.logp = -0.5 * res * res / aux;
    }
    T.D = fmax(T.D, 0x1p-40);
    return T;
}

// One Newton linearisation at x (x_in: the start, or the mean of the last pass): pseudo-observations t = x + g / D into y, their
// noise r = 1 / D and sqrt(r) into noise / noise_sd, and x into x_keep (the reduction takes the step against it).  Rows the plan does
// not observe keep their y and get r = 0.  The Gaussian family's t = z - offset and r = aux do not depend on x and are written as
// such, so that the plan holds exactly what set_obs(z - offset) + set_noise(aux) leave.  x_in may be x_keep itself (same index read
// and written by one thread).
__global__ __launch_bounds__(256) void k_laplace_linearise(int family, const double* __restrict__ z, const double* __restrict__ aux,
                                                           const double* __restrict__ off, const double* x_in, double* x_keep,
                                                           double* __restrict__ y, double* __restrict__ noise, double* __restrict__ noise_sd, long P) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const double zp = z[p];
    if (!(fabs(zp) < __builtin_inf())) { noise[p] = 0.0; noise_sd[p] = 0.0; x_keep[p] = 0.0; return; }
    const double x = x_in[p], a = aux[p], o = off[p];
    double t, r;
    if (family == MRA_FAMILY_GAUSSIAN) {
        t = zp - o;
        r = (1.0 / a >= 0x1p-40) ? a : 0x1p40;
    } else {
        const LaplaceTerm T = laplace_term(family, zp, a, x + o);
        t = x + T.g / T.D;
        r = 1.0 / T.D;
    }
    x_keep[p] = x;
    y[p] = t; noise[p] = r; noise_sd[p] = sqrt(r);
}

// a workgroup's 256 x LAPLACE_NRES values -> its partial results: a fixed tree, the two maxima first (they keep a NaN)
__device__ __forceinline__ void laplace_fold(const double (&v)[LAPLACE_NRES], double (&sh)[LAPLACE_NRES][256], double* __restrict__ part) {
#pragma unroll
    for (int k = 0; k < LAPLACE_NRES; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < LAPLACE_NRES; ++k) {
                const double a = sh[k][threadIdx.x], b = sh[k][threadIdx.x + w];
                sh[k][threadIdx.x] = k < 2 ? laplace_max(a, b) : a + b;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < LAPLACE_NRES) part[(long)blockIdx.x * LAPLACE_NRES + threadIdx.x] = sh[threadIdx.x][0];
}

// After the pass: with x^ = mean at the observed rows, per workgroup {max |x^ - x|, max |x^|, sum log D, sum D (t - x^)^2, sum of the
// x-dependent part of log p(z | x^ + offset)}, D = 1 / noise and t = y of the pass.  A thread walks its rows in order, the workgroup
// folds its 256 values in a fixed tree: the same inputs give the same bits.  The two maxima keep a NaN (laplace_max): a mean that is
// not finite at an observed row gives a step that is not finite.
__global__ __launch_bounds__(256) void k_laplace_part(int family, const double* __restrict__ z, const double* __restrict__ aux,
                                                      const double* __restrict__ off, const double* __restrict__ x_keep,
                                                      const double* __restrict__ mean, const double* __restrict__ y,
                                                      const double* __restrict__ noise, long P, double* __restrict__ part) {
    __shared__ double sh[LAPLACE_NRES][256];
    double v[LAPLACE_NRES] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
        const double zp = z[p];
        if (!(fabs(zp) < __builtin_inf())) continue;
        const double xh = mean[p], D = 1.0 / noise[p], dt = y[p] - xh;
        v[0] = laplace_max(v[0], fabs(xh - x_keep[p]));
        v[1] = laplace_max(v[1], fabs(xh));
        v[2] += log(D);
        v[3] += D * dt * dt;
        v[4] += laplace_term(family, zp, aux[p], xh + off[p]).logp;
    }
    laplace_fold(v, sh, part);
}

// ---- mra_plan_fit_laplace_trend: the tail of one iteration with a regression trend ------------------------------
// m: (1 + p) x P zero-mean kriging means of [t | X] (row 0: m_t), X: p x P design matrix, both by padded row; beta: the GLS estimate
// of this pass.  At every observed row e^ = m_t + (X - m_X)^T beta^ (the sum in k_trend_rows' order) replaces the iterate in x - read
// first: the step is taken against it - and the workgroup's five partial results are those of k_laplace_part with x^ := e^: same
// number of workgroups, same walk, same fold, so k_laplace_sum finishes both.  One row per lane: covariate j of 64 consecutive rows
// is one 512-byte line of X and one of m; beta^ sits in LDS and is read by broadcast; no per-lane array.
__global__ __launch_bounds__(256) void k_laplace_trend_part(int family, const double* __restrict__ z, const double* __restrict__ aux,
                                                            const double* __restrict__ off, double* __restrict__ x,
                                                            const double* __restrict__ m, const double* __restrict__ X,
                                                            const double* __restrict__ beta, const double* __restrict__ y,
                                                            const double* __restrict__ noise, int p, long P, double* __restrict__ part) {
    __shared__ double sh[LAPLACE_NRES][256];
    __shared__ double bs[64];
    if (threadIdx.x < 64) bs[threadIdx.x] = (int)threadIdx.x < p ? beta[threadIdx.x] : 0.0;
    __syncthreads();
    double v[LAPLACE_NRES] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < P; s += (long)gridDim.x * 256) {
        const double zp = z[s];
        if (!(fabs(zp) < __builtin_inf())) continue;
        double eh = m[s];
#pragma unroll 4
        for (int j = 0; j < p; ++j) eh = __builtin_fma(X[(long)j * P + s] - m[(long)(j + 1) * P + s], bs[j], eh);
        const double D = 1.0 / noise[s], dt = y[s] - eh;
        v[0] = laplace_max(v[0], fabs(eh - x[s]));
        v[1] = laplace_max(v[1], fabs(eh));
        v[2] += log(D);
        v[3] += D * dt * dt;
        v[4] += laplace_term(family, zp, aux[s], eh + off[s]).logp;
        x[s] = eh;
    }
    laplace_fold(v, sh, part);
}

// the workgroups' partial results -> res[LAPLACE_NRES]: one wave per result; lane l folds workgroups l, l + 64, ... in that order, then
// the 64 lanes fold in a fixed tree
__global__ __launch_bounds__(64 * LAPLACE_NRES) void k_laplace_sum(const double* __restrict__ part, int nblk, double* __restrict__ res) {
    __shared__ double sh[LAPLACE_NRES][64];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int b = lane; b < nblk; b += 64) {
        const double a = part[(long)b * LAPLACE_NRES + k];
        acc = k < 2 ? laplace_max(acc, a) : acc + a;
    }
    sh[k][lane] = acc;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if (lane < w) {
            const double a = sh[k][lane], b = sh[k][lane + w];
            sh[k][lane] = k < 2 ? laplace_max(a, b) : a + b;
        }
        __syncthreads();
    }
    if (lane == 0) res[k] = sh[k][0];
}
