// mra_cov_kernels.h - kernels of mra_cov_apply: the MRA prior covariance of the reported rows,
//     Sigma = sum over non-leaf j of W_j W_j^T + sum over leaves l of v_M(K_l, K_l),   v_M(S, S) = C(S, S) - W_anc[S] W_anc[S]^T,
// applied to a block of 16 vectors from the whitened basis W a likelihood pass with W at every row left in the plan.  Included by
// mra_launch_cov.hip only, so that the other translation units keep their object code.
//
// The in / out blocks Ab and out are 16 x P (vector c at + c P, padded leaf order), as mra_solve's; the work arrays are row-major
// with 16 doubles per row ("x16").  Abar = rep o A (the reported rows), Acheck = knot o Abar (the knot rows of a row's own leaf):
// masks are applied by selection, never by a product, so that NaN at rows that are not read stays out.
// MFMA conventions (mra_kernels.h): lane (r, q) = (lane & 15, lane >> 4); mfma16(a, b, acc) over k-step s takes a = A[r][q + 4 s],
// b = B[q + 4 s][r] and leaves D[q + 4 j][r] in acc[j].
#pragma once
#include "mra_plan_types.h"      // CovLeaf, SolveFront; mra_kernels.h

static const int COV_GRAM_BLOCKS = 512;

// ---- 1. leaves: t = W[S, anc]^T Abar[S], t' = W[S, anc]^T Acheck[S] (anc x16 each), one workgroup of four waves per leaf -----------
// W tiles transposed as the A operand (lane (r, q) reads W[row q + 4 s][column r]: 16 consecutive doubles per q), the k loop over
// the leaf's row tiles.  anc == 0 (a single-leaf tree): nothing is read or written.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_cov.hip */
__global__ __launch_bounds__(256, 4) void k_cov_leaf_proj(const CovLeaf* __restrict__ lv, const double* __restrict__ W, long ldw,
                                                          const double* __restrict__ Ab, const unsigned char* __restrict__ rep,
                                                          const unsigned char* __restrict__ knot, long P) {
    const CovLeaf L = lv[blockIdx.x];
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    for (int at = threadIdx.x >> 6; at < (L.anc >> 4); at += 4) {
        d4 acc = {0, 0, 0, 0}, accp = {0, 0, 0, 0};
        for (int k0 = 0; k0 < L.nrows; k0 += 16) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const long row = L.row0 + k0 + q + 4 * s;
                const bool rp = rep[row] != 0, kn = rp && knot[row] != 0;
                const double w = gld(W + row * ldw + L.a0 + at * 16 + r);
                const double v = gld(Ab + (long)r * P + row);
                const double a = rp ? w : 0.0;
                acc = mfma16(a, rp ? v : 0.0, acc);
                accp = mfma16(a, kn ? v : 0.0, accp);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            gst(L.t + (long)(at * 16 + q + 4 * j) * 16 + r, acc[j]);
            gst(L.tp + (long)(at * 16 + q + 4 * j) * 16 + r, accp[j]);
        }
    }
}
#endif

// ---- 2. fronts, bottom-up, one workgroup per node, one launch per level: buf <- sum over the children's chain buffers, in child-list
// order.  Rows [0, cw) are the node's own tau_j = W_j^T Abar[rows_j]; rows [cw, cw + anc) go on to the parent.  Sums only.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_cov.hip */
__global__ __launch_bounds__(256) void k_cov_up(const SolveFront* __restrict__ fv, const double* const* __restrict__ kids) {
    const SolveFront N = fv[blockIdx.x];
    const int nall = (N.cw + N.anc) * 16;
    for (int e = threadIdx.x; e < nall; e += 256) {
        double f = 0.0;
        for (int k = 0; k < N.nkid; ++k) f += gld(kids[N.kid0 + k] + e);
        gst(N.buf + e, f);
    }
}
#endif

// ---- 3. fronts, top-down: buf <- [tau_j ; tau_chain], tau_chain = the parent's whole buffer (the layout of mra_solve's [alpha ; chain])
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_cov.hip */
__global__ __launch_bounds__(256) void k_cov_down(const SolveFront* __restrict__ fv) {
    const SolveFront N = fv[blockIdx.x];
    const int nown = N.cw * 16, nall = (N.cw + N.anc) * 16;
    for (int e = nown + threadIdx.x; e < nall; e += 256) gst(N.buf + e, gld(N.chain + (e - nown)));
}
#endif

// ---- 4. rows, one wave per 16-row tile:
//     out[tile] = rep o ( W[tile, anc] tau_chain + knot o ( C(tile, S_l) Acheck[S_l] - W[tile, anc] t'_l ) )
// W in row-on-lane form as k_sample_coarse; the kernel values C(x_row r, x_k) computed by the lane that needs them as the A operand,
// as k_solve_rows does.  A tile without a knot row skips the second term, a row tile of S_l without a knot row its 16 columns.
// Every row read lies inside the leaf [row0, row0 + nrows).
template <int MODE>
__device__ __forceinline__ double cov_value(const KernelParams& kp, double D2) {
    if (MODE == 3) {             // the Kanter taper through sinpi / cospi (no range-reduction table on the stack), as k_solve_rows
        const double D = fmin(sqrt_pos(D2) * kp.c_inv_l, 2.0);
        const double p2 = 6.283185307179586 * D;
        const double v = (1.0 - D) * sinpi(2.0 * D) / p2 + 0.3183098861837907 * (1.0 - cospi(2.0 * D)) / p2;
        return kp.amp * ((D == 0.0) ? 1.0 : ((D > 1.0) ? 0.0 : v));
    }
    return cov_of_dist2<MODE>(kp, D2);
}

// ... of a pair of locations: the same expression as before for the modes that are functions of the distance, cov_local for mode 6
template <int DIM, int MODE>
__device__ __forceinline__ double cov_value_pair(const KernelParams& kp, const double* __restrict__ xa, const double* __restrict__ xb) {
    if constexpr (MODE == 6) return cov_local<DIM>(kp, xa, xb);
    else return cov_value<MODE>(kp, pair_dist2<DIM>(xa, xb, kp.circular));
}

template <int DIM, int MODE>
__global__ __launch_bounds__(256, 4) void k_cov_rows(const CovLeaf* __restrict__ lv, const int* __restrict__ tile_leaf,
                                                     const double* __restrict__ W, long ldw, const double* __restrict__ X,
                                                     const unsigned char* __restrict__ rep, const unsigned char* __restrict__ knot,
                                                     KernelParams kp, const double* __restrict__ Ab, double* __restrict__ out, long P) {
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 16 >= P) return;
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const long row0 = tile * 16;
    d4 acc = {0, 0, 0, 0}, accl = {0, 0, 0, 0};
    const int t = tile_leaf[tile];
    if (t >= 0) {
        const CovLeaf L = lv[t];
        const bool leaf_term = __ballot(rep[row0 + r] && knot[row0 + r]) != 0;
        for (int k0 = 0; k0 < L.anc; k0 += 16) {
            const d4 a = load_rowlane(W + row0 * ldw + L.a0 + k0, ldw, r, q);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc = mfma16(a[s], gld(L.chain + (long)(k0 + q + 4 * s) * 16 + r), acc);
                if (leaf_term) accl = mfma16(-a[s], gld(L.tp + (long)(k0 + q + 4 * s) * 16 + r), accl);
            }
        }
        if (leaf_term) {
            double xr[DIM];
#pragma unroll
            for (int e = 0; e < DIM; ++e) xr[e] = gld(X + (row0 + r) * DIM + e);
            for (int k0 = 0; k0 < L.nrows; k0 += 16) {
                const long kr = L.row0 + k0 + r;
                if (__ballot(rep[kr] && knot[kr]) == 0) continue;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const long k = L.row0 + k0 + q + 4 * s;
                    const bool kn = rep[k] && knot[k];
                    double xk[DIM];
#pragma unroll
                    for (int e = 0; e < DIM; ++e) xk[e] = gld(X + k * DIM + e);
                    const double cv = cov_value_pair<DIM, MODE>(kp, xr, xk);
                    const double v = gld(Ab + (long)r * P + k);
                    accl = mfma16(kn ? cv : 0.0, kn ? v : 0.0, accl);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long row = row0 + q + 4 * j;
        gst(out + (long)r * P + row, rep[row] ? acc[j] + (knot[row] ? accl[j] : 0.0) : 0.0);
    }
}

// ---- 5. posterior: Sigma_post A = Sigma A - mean_MRA((Sigma A)_o).  The right-hand sides of mra_solve's sweeps are read at observed rows
// only, so the block is copied whole; the mean comes back in the solver's out block.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_cov.hip */
__global__ __launch_bounds__(256) void k_cov_to_rhs(const double* __restrict__ out, double* __restrict__ yb, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) yb[i] = out[i];
}
__global__ __launch_bounds__(256) void k_cov_sub(double* __restrict__ out, const double* __restrict__ mean,
                                                 const unsigned char* __restrict__ rep, long P) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || !rep[p]) return;
    for (int c = 0; c < 16; ++c) out[(long)c * P + p] -= mean[(long)c * P + p];
}
#endif

// ---- 6. gram = Abar out^T (16 x 16) over COV_GRAM_BLOCKS partial sums in a fixed order.  Workgroup b takes the row tiles
// [b nt, (b + 1) nt), its wave w every fourth of them on the MFMA (A = Abar as 16 x k, B = out^T: both operands are read in the same
// form, vector r at row q + 4 s); the four waves' sums are added in wave order.  part: [block][i * 16 + j].
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_cov.hip */
__global__ __launch_bounds__(256, 4) void k_cov_gram_part(const double* __restrict__ Ab, const double* __restrict__ out,
                                                          const unsigned char* __restrict__ rep, long P, long nt,
                                                          double* __restrict__ part) {
    __shared__ double red[4][256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const long t1 = min((long)(blockIdx.x + 1) * nt, P / 16);
    d4 acc = {0, 0, 0, 0};
    for (long tile = (long)blockIdx.x * nt + w; tile < t1; tile += 4) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long row = tile * 16 + q + 4 * s;
            const bool rp = rep[row] != 0;
            const double a = gld(Ab + (long)r * P + row), b = gld(out + (long)r * P + row);
            acc = mfma16(rp ? a : 0.0, rp ? b : 0.0, acc);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[w][(q + 4 * j) * 16 + r] = acc[j];
    __syncthreads();
    part[(long)blockIdx.x * 256 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}
#endif
// Sigma is symmetric, the two roundings of an entry and its mirror image are not: the mean of the two is returned.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_cov.hip */
__global__ __launch_bounds__(256) void k_cov_gram_sum(const double* __restrict__ part, int nblk, double* __restrict__ gram) {
    __shared__ double g[256];
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b) acc += part[(long)b * 256 + threadIdx.x];
    g[threadIdx.x] = acc;
    __syncthreads();
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    gram[threadIdx.x] = 0.5 * (g[i * 16 + j] + g[j * 16 + i]);
}
#endif
