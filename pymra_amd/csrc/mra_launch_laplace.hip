// mra_launch_laplace.hip - mra_plan_fit_laplace: the work buffers and the launches between two passes of the
// Newton iteration.  A translation unit of its own: the kernels of the pass keep their object code.
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
