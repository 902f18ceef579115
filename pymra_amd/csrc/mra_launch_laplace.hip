// mra_launch_laplace.hip - mra_plan_fit_laplace and mra_plan_fit_laplace_trend (section 21): the work buffers and
// the launches between two passes of the Newton iteration - and the other elementwise kernel of the library, k_metric_apply of
// mra_plan_set_metric, at the end.  A translation unit of its own: the kernels of the pass keep their object code.
#define MRA_KERNELS_TEMPLATES_ONLY
#include "mra_laplace_kernels.h"

void mra_laplace_reserve(mra_plan* pl) {
    mra_plan::Laplace& L = pl->lap;
    const size_t P = (size_t)pl->P;
    if (L.z.n != P) { L.z.alloc(P); L.aux.alloc(P); L.off.alloc(P); L.x.alloc(P); }
    if (!L.part.n) { L.part.alloc((size_t)LAPLACE_BLOCKS * LAPLACE_NRES); }
    if (pl->noise.n != P) { pl->noise.alloc(P); pl->noise_sd.alloc(P); }
}

void mra_laplace_linearise(mra_plan* pl, int family, const double* x_in) {
    mra_plan::Laplace& L = pl->lap;
    hipLaunchKernelGGL(k_laplace_linearise, dim3((unsigned)((pl->P + 255) / 256)), dim3(256), 0, pl->stream, family, L.z.p, L.aux.p, L.off.p,
                       x_in, L.x.p, pl->y.p, pl->noise.p, pl->noise_sd.p, pl->P);
}

void mra_laplace_reduce(mra_plan* pl, int family, double* res) {
    mra_plan::Laplace& L = pl->lap;
    static_assert(LAPLACE_NRES == MRA_LAPLACE_NRES, "the plan's record and the kernels disagree");
    hipLaunchKernelGGL(k_laplace_part, dim3(LAPLACE_BLOCKS), dim3(256), 0, pl->stream, family, L.z.p, L.aux.p, L.off.p, L.x.p, pl->mean.p,
                       pl->y.p, pl->noise.p, pl->P, L.part.p);
    hipLaunchKernelGGL(k_laplace_sum, dim3(1), dim3(64 * LAPLACE_NRES), 0, pl->stream, L.part.p, LAPLACE_BLOCKS, res);
}

// mra_plan_fit_laplace_trend: e^ from trend.m, trend.X and beta (device, trend.coef) into lap.x, and the five results of the iteration
void mra_laplace_trend_reduce(mra_plan* pl, int family, double* res) {
    mra_plan::Laplace& L = pl->lap;
    mra_plan::Trend& T = pl->trend;
    hipLaunchKernelGGL(k_laplace_trend_part, dim3(LAPLACE_BLOCKS), dim3(256), 0, pl->stream, family, L.z.p, L.aux.p, L.off.p, L.x.p, T.m.p,
                       T.X.p, T.coef.p, pl->y.p, pl->noise.p, T.p, pl->P, L.part.p);
    hipLaunchKernelGGL(k_laplace_sum, dim3(1), dim3(64 * LAPLACE_NRES), 0, pl->stream, L.part.p, LAPLACE_BLOCKS, res);
}

// ---- mra_plan_set_metric: X = A Xraw, once per change of A, in front of every kernel that reads coordinates ----
// One row per lane; A arrives in the kernel arguments (scalar registers); a 2-D row is one 16-byte load and one 16-byte store.
struct MetricA { double a[9]; };
template <int DIM>
__global__ __launch_bounds__(256) void k_metric_apply(MetricA A, const double* __restrict__ raw, double* __restrict__ X, long P) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double x[DIM], t[DIM];
    if (DIM == 2) { const double2 v = reinterpret_cast<const double2*>(raw)[p]; x[0] = v.x; x[DIM - 1] = v.y; }
    else {
#pragma unroll
        for (int k = 0; k < DIM; ++k) x[k] = raw[p * DIM + k];
    }
    mra_metric_row<DIM>(A.a, x, t);
    if (DIM == 2) reinterpret_cast<double2*>(X)[p] = make_double2(t[0], t[DIM - 1]);
    else {
#pragma unroll
        for (int k = 0; k < DIM; ++k) X[p * DIM + k] = t[k];
    }
}

void mra_metric_apply(mra_plan* pl) {
    const long P = pl->P;
    const int d = pl->d;
    if (g_dry) {                                          // host dry run: the buffers are host memory
        for (long p = 0; p < P; ++p) mra_metric_row_d(d, pl->metric_A, pl->Xraw.p + p * d, pl->X.p + p * d);
        return;
    }
    MetricA A;
    for (int k = 0; k < d * d; ++k) A.a[k] = pl->metric_A[k];
    for (int k = d * d; k < 9; ++k) A.a[k] = 0.0;
    const dim3 grid((unsigned)((P + 255) / 256)), block(256);
    if (d == 1) hipLaunchKernelGGL(k_metric_apply<1>, grid, block, 0, pl->stream, A, pl->Xraw.p, pl->X.p, P);
    else if (d == 2) hipLaunchKernelGGL(k_metric_apply<2>, grid, block, 0, pl->stream, A, pl->Xraw.p, pl->X.p, P);
    else hipLaunchKernelGGL(k_metric_apply<3>, grid, block, 0, pl->stream, A, pl->Xraw.p, pl->X.p, P);
}
