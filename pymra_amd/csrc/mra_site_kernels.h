// mra_site_kernels.h - kernels of mra_predict_sites: the posterior mean and variance of the MRA process at
// locations that are not rows of the tree, from the state one likelihood pass leaves in the plan (the prior W and factors L_j, the
// leaves' L_c and Ut, the fronts' Lt and Zt) and, for the mean, the beta / q of the solver's backward sweep.  Included by
// mra_launch_sites.hip only, so that the other translation units keep their object code.  The last kernel, k_site_gram, is
// mra_sites_cov's (section 13): the joint covariance of the sites of two tiles from the arrays the first three leave behind.  After it,
// the kernels of mra_sample_sites (section 14): the inert flags, the leaves' blocks G_l, the staged leaf draws and the draw itself.
// Last, the kernels of mra_cv (section 18): the observed rows as sites, the groups' blocks N_G, their solves and the reduction.
//
// A tile is 16 sites of ONE leaf; the 16 sites are the 16 columns (N) of v_mfma_f64_16x16x4_f64 throughout, so a^T, t, b and p_j are
// k x16 arrays in the solver's "x16" layout: element (row, site) at row * 16 + site.  Every column of an MFMA product, of a
// substitution and of a column sum depends on that column's operands alone and is summed in an order that depends on the plan alone:
// the result for a site is a pure function of (site, leaf, plan state), whatever shares its tile.
// One wave per tile (workgroups of 64): the tiles of a leaf are neighbours in the grid, so L_c and Ut are served by the caches after
// the first of them.  MFMA conventions as in mra_solve_kernels.h: lane (r, q) = (lane & 15, lane >> 4); mfma16(a, b, acc) over k-step
// s takes a = A[r][q + 4 s], b = B[q + 4 s][r] and leaves D[q + 4 j][r] in acc[j].
#pragma once
#include "mra_plan_types.h"      // SolveLeaf, SiteNode; mra_kernels.h

template <int MODE>
__device__ __forceinline__ double site_cov(const KernelParams& kp, double D2) {
    if (MODE == 3) {             // the Kanter taper through sinpi / cospi (no range-reduction table on the stack), as k_solve_rows
        const double D = fmin(sqrt_pos(D2) * kp.c_inv_l, 2.0);
        const double p2 = 6.283185307179586 * D;
        const double v = (1.0 - D) * sinpi(2.0 * D) / p2 + 0.3183098861837907 * (1.0 - cospi(2.0 * D)) / p2;
        return kp.amp * ((D == 0.0) ? 1.0 : ((D > 1.0) ? 0.0 : v));
    }
    return cov_of_dist2<MODE>(kp, D2);
}

// x <- L^-1 rhs for a lower-triangular L (n = 16 nt rows, row stride ld; only its lower triangle is read) and 16 columns, x in the
// x16 layout.  rhs(I) gives rows I * 16 + q + 4 j of column r in element j; it may read x's own tile I (in-place solve).  Off-diagonal
// tiles on the MFMA, the 16 x 16 diagonal block by substitution across the wave (the block in LDS, the solved row broadcast with one
// shuffle per step) - k_solve_leaf_trsm<false>.  Ld: 256 doubles of LDS.  Ends with x visible to the whole wave.
template <class RHS>
__device__ __forceinline__ void site_trsm(const double* __restrict__ L, int ld, int nt, double* __restrict__ x, double* Ld, RHS rhs) {
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    for (int I = 0; I < nt; ++I) {
        d4 acc = rhs(I);
        for (int J = 0; J < I; ++J) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = J * 16 + q + 4 * s;
                acc = mfma16(-gld(L + (long)(I * 16 + r) * ld + k), gld(x + (long)k * 16 + r), acc);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) Ld[lane + 64 * j] = gld(L + (long)(I * 16 + q + 4 * j) * ld + I * 16 + r);
        __syncthreads();
        // Ld[i * 16 + k] = L_II[i][k]; lane (r, q) holds rows q + 4 j of column r
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const double xk = __shfl(acc[k >> 2], r + 16 * (k & 3), 64) / Ld[k * 17];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = q + 4 * j;
                if (row > k) acc[j] = __builtin_fma(-Ld[row * 16 + k], xk, acc[j]);
                if (row == k) acc[j] = xk;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) gst(x + (long)(I * 16 + q + 4 * j) * 16 + r, acc[j]);
        __syncthreads();             // the tile is read back by every lane of the wave in the next steps
    }
}

// sum over the n rows of an x16 array of the squares, per column: the lane's quarter of the rows (k = q mod 4, ascending), then the
// four quarters in a fixed order.  Every lane of column r gets the sum.
__device__ __forceinline__ double site_colsq(const double* __restrict__ x, int n, int r, int q) {
    double s = 0.0;
    for (int k = q; k < n; k += 4) { const double v = gld(x + (long)k * 16 + r); s = __builtin_fma(v, v, s); }
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    return s;
}

// ---- 1. basis: a(s), top-down along the leaf's chain ---------------------------------------------------------------------------------
// a_k = L_k^-1 (C(Q_k, s) - W[Q_k, ancestors of k] a_{<k}), the row recursion of the prior for a location that is not a row: knot
// coordinates and W rows are gathered through the node's knot list; a phantom knot gives 0.  The covariance value is computed by the
// lane that holds the element (knot q + 4 j of the tile, site r).
// C(x, x): the kernel at distance 0, as before; mode 6 is exactly amp there whatever the range (cov_local_of)
template <int MODE>
__device__ __forceinline__ double site_cov0(const KernelParams& kp) {
    if constexpr (MODE == 6) return kp.amp;
    else return site_cov<MODE>(kp, 0.0);
}
// ... of a pair of locations: the same expression as before for the modes that are functions of the distance, cov_local for mode 6
template <int DIM, int MODE>
__device__ __forceinline__ double site_cov_pair(const KernelParams& kp, const double* __restrict__ xa, const double* __restrict__ xb) {
    if constexpr (MODE == 6) return cov_local<DIM>(kp, xa, xb);
    else return site_cov<MODE>(kp, pair_dist2<DIM>(xa, xb, kp.circular));
}

template <int DIM, int MODE>
__global__ __launch_bounds__(64, 4) void k_site_basis(const SolveLeaf* __restrict__ lv, const SiteNode* __restrict__ nodes,
                                                      const int* __restrict__ chain_ptr, const int* __restrict__ chain,
                                                      const int* __restrict__ tile_leaf, const double* __restrict__ xs,
                                                      const double* __restrict__ W, long ldw, const double* __restrict__ X,
                                                      KernelParams kp, double* __restrict__ a_buf, long a_stride) {
    __shared__ double Ld[256];
    const long tile = blockIdx.x;
    const int t = tile_leaf[tile];
    const SolveLeaf L = lv[t];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    double* a = a_buf + tile * a_stride;
    double xr[DIM];
#pragma unroll
    for (int e = 0; e < DIM; ++e) xr[e] = gld(xs + (tile * 16 + r) * DIM + e);
    const int c0 = chain_ptr[t], c1 = chain_ptr[t + 1];
    for (int c = c0; c < c1; ++c) {
        const SiteNode N = nodes[chain[c]];
        const int own = N.c0 - L.a0, up = own + N.cw;          // the node's own block and its ancestors' blocks in a
        const double* Wup = W + N.c0 + N.cw;
        site_trsm(N.Lp, N.cw, N.cw >> 4, a + (long)own * 16, Ld, [&](int I) {
            d4 acc;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kn = gldi(N.knots + I * 16 + q + 4 * j);
                double xk[DIM];
#pragma unroll
                for (int e = 0; e < DIM; ++e) xk[e] = gld(X + (long)(kn >= 0 ? kn : 0) * DIM + e);
                const double cv = site_cov_pair<DIM, MODE>(kp, xk, xr);
                acc[j] = kn >= 0 ? cv : 0.0;
            }
            const int kr = gldi(N.knots + I * 16 + r);
            const double* wrow = Wup + (long)(kr >= 0 ? kr : 0) * ldw;
            for (int k0 = 0; k0 < N.anc; k0 += 16) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = k0 + q + 4 * s;
                    const double w = gld(wrow + k);
                    acc = mfma16(kr >= 0 ? -w : 0.0, gld(a + (long)(up + k) * 16 + r), acc);
                }
            }
            return acc;
        });
    }
}

// ---- 2. leaf: t = L_c^-1 C(o, s) - Ut_anc^T a, b = a - Ut_anc t, v = max(C(s, s) - |a|^2 - |t|^2, 0) ---------------------------------
// The substitution is k_solve_leaf_trsm<false>'s, the two Ut products are k_solve_leaf_sbeta's.  Phantom observations contribute 0.
template <int DIM, int MODE>
__global__ __launch_bounds__(64, 4) void k_site_leaf(const SolveLeaf* __restrict__ lv, const int* __restrict__ tile_leaf,
                                                     const double* __restrict__ xs, const double* __restrict__ X, KernelParams kp,
                                                     const double* __restrict__ a_buf, double* __restrict__ b_buf, long a_stride,
                                                     double* __restrict__ t_buf, long t_stride, double* __restrict__ var) {
    __shared__ double Ld[256];
    const long tile = blockIdx.x;
    const SolveLeaf L = lv[tile_leaf[tile]];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4, nop = L.nop, anc = L.anc;
    const double* a = a_buf + tile * a_stride;
    double* b = b_buf + tile * a_stride;
    double* tt = t_buf + tile * t_stride;
    double xr[DIM];
#pragma unroll
    for (int e = 0; e < DIM; ++e) xr[e] = gld(xs + (tile * 16 + r) * DIM + e);
    site_trsm(L.Lc, nop, nop >> 4, tt, Ld, [&](int I) {
        d4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = gldi(L.obs + I * 16 + q + 4 * j);
            double xo[DIM];
#pragma unroll
            for (int e = 0; e < DIM; ++e) xo[e] = gld(X + (long)(o >= 0 ? o : 0) * DIM + e);
            const double cv = site_cov_pair<DIM, MODE>(kp, xo, xr);
            acc[j] = o >= 0 ? cv : 0.0;
        }
        return acc;
    });
    for (int ot = 0; ot < (nop >> 4); ++ot) {
        d4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = gld(tt + (long)(ot * 16 + q + 4 * j) * 16 + r);
        for (int a0 = 0; a0 < anc; a0 += 16) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = a0 + q + 4 * s;
                acc = mfma16(-gld(L.Ut + (long)k * nop + ot * 16 + r), gld(a + (long)k * 16 + r), acc);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = ot * 16 + q + 4 * j;
            gst(tt + (long)k * 16 + r, gldi(L.obs + k) >= 0 ? acc[j] : 0.0);
        }
    }
    __syncthreads();
    for (int at = 0; at < (anc >> 4); ++at) {
        d4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = gld(a + (long)(at * 16 + q + 4 * j) * 16 + r);
        for (int o0 = 0; o0 < nop; o0 += 16) {
            const d4 u = load_rowlane(L.Ut + (long)at * 16 * nop + o0, nop, r, q);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma16(-u[s], gld(tt + (long)(o0 + q + 4 * s) * 16 + r), acc);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) gst(b + (long)(at * 16 + q + 4 * j) * 16 + r, acc[j]);
    }
    const double v = site_cov0<MODE>(kp) - site_colsq(a, anc, r, q) - site_colsq(tt, nop, r, q);
    if (q == 0) gst(var + tile * 16 + r, fmax(v, 0.0));
}

// ---- 3. chain: parent up to root, p_j = Lt_j^-1 b[own], b[ancestors of j] -= Zt_j p_j, var += |p_j|^2 --------------------------------
// The solver's forward sweep (k_solve_front_fwd) on one chain, in place in b.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(64, 4) void k_site_chain(const SolveLeaf* __restrict__ lv, const SiteNode* __restrict__ nodes,
                                                      const int* __restrict__ chain_ptr, const int* __restrict__ chain,
                                                      const int* __restrict__ tile_leaf, double* __restrict__ b_buf, long a_stride,
                                                      double* __restrict__ var) {
    __shared__ double Ld[256];
    const long tile = blockIdx.x;
    const int t = tile_leaf[tile];
    const SolveLeaf L = lv[t];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    double* b = b_buf + tile * a_stride;
    double v = 0.0;
    const int c0 = chain_ptr[t], c1 = chain_ptr[t + 1];
    for (int c = c1 - 1; c >= c0; --c) {
        const SiteNode N = nodes[chain[c]];
        double* p = b + (long)(N.c0 - L.a0) * 16;
        double* up = p + (long)N.cw * 16;
        site_trsm(N.F, N.ld, N.cw >> 4, p, Ld, [&](int I) {
            d4 acc;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = gld(p + (long)(I * 16 + q + 4 * j) * 16 + r);
            return acc;
        });
        for (int at = 0; at < (N.anc >> 4); ++at) {
            d4 acc;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = gld(up + (long)(at * 16 + q + 4 * j) * 16 + r);
            for (int k0 = 0; k0 < N.cw; k0 += 16) {
                const d4 z = load_rowlane(N.F + (long)(N.cw + at * 16) * N.ld + k0, N.ld, r, q);
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = mfma16(-z[s], gld(p + (long)(k0 + q + 4 * s) * 16 + r), acc);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) gst(up + (long)(at * 16 + q + 4 * j) * 16 + r, acc[j]);
        }
        __syncthreads();
        v += site_colsq(p, N.cw, r, q);
    }
    if (q == 0) gst(var + tile * 16 + r, gld(var + tile * 16 + r) + v);
}
#endif

// ---- 4. mean: mean[site, 0:16] = a(site)^T beta + C(site, o) q ------------------------------------------------------------------------
// k_solve_rows with a(s) in place of a row of W: the 16 sites are the M side here, the 16 observation vectors the N side.  Columns
// < n_cols are written: out[c * ldo + tile * 16 + site].
template <int DIM, int MODE>
__global__ __launch_bounds__(64, 4) void k_site_mean(const SolveLeaf* __restrict__ lv, const int* __restrict__ tile_leaf,
                                                     const double* __restrict__ xs, const double* __restrict__ X, KernelParams kp,
                                                     const double* __restrict__ a_buf, long a_stride, int n_cols,
                                                     double* __restrict__ out, long ldo) {
    const long tile = blockIdx.x;
    const SolveLeaf L = lv[tile_leaf[tile]];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const double* a = a_buf + tile * a_stride;
    d4 acc = {0, 0, 0, 0};
    for (int k0 = 0; k0 < L.anc; k0 += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = k0 + q + 4 * s;
            acc = mfma16(gld(a + (long)k * 16 + r), gld(L.gb + (long)k * 16 + r), acc);
        }
    }
    double xr[DIM];
#pragma unroll
    for (int e = 0; e < DIM; ++e) xr[e] = gld(xs + (tile * 16 + r) * DIM + e);
    for (int o0 = 0; o0 < L.nop; o0 += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = o0 + q + 4 * s;
            const int o = gldi(L.obs + k);
            double xo[DIM];
#pragma unroll
            for (int e = 0; e < DIM; ++e) xo[e] = gld(X + (long)(o >= 0 ? o : 0) * DIM + e);
            const double cv = site_cov_pair<DIM, MODE>(kp, xr, xo);
            acc = mfma16(o >= 0 ? cv : 0.0, gld(L.uy + (long)k * 16 + r), acc);
        }
    }
    if (r < n_cols) {
#pragma unroll
        for (int j = 0; j < 4; ++j) gst(out + (long)r * ldo + tile * 16 + q + 4 * j, acc[j]);
    }
}

// ---- 5. gram: the joint covariance of the sites of two tiles (mra_sites_cov) -------------------------------------
// One wave per 16 x 16 block (tile I = blockIdx.y + tile0, tile J = blockIdx.x; blocks with J < I are the caller's to mirror and are
// not computed): the 16 sites of I are M, those of J are N.  W's columns run deepest block first and end at Ka for every leaf, so the
// blocks of the two leaves' common ancestors are the trailing w = cw + anc rows (of the lowest common ancestor's SiteNode) of both
// tiles' arrays, and the cross term is one product over a contiguous K range, ascending:
//     prior      different leaves: sum_k a_I[k] a_J[k]           same leaf: C(s_u, s_w)
//     posterior  different leaves: sum_k p_I[k] p_J[k]           same leaf: sum_k p p - sum_k a a (anc) - sum_k t t (nop) + C(s_u, s_w)
// (p: k_site_chain's b).  Both operands of a k-step are rows of x16 arrays, so element (u, w) is the same chain of fused
// multiply-adds whichever of the two sites is on the M side: the block of (J, I) is the transpose of this one to the bit.
// Lane (r, q) leaves elements (q + 4 j, r); out has row stride ldo, row 0 = site 0 of tile tile0.
template <int DIM, int MODE, bool POST>
__global__ __launch_bounds__(64, 4) void k_site_gram(const SolveLeaf* __restrict__ lv, const SiteNode* __restrict__ nodes,
                                                     const int* __restrict__ chain_ptr, const int* __restrict__ chain,
                                                     const int* __restrict__ tile_leaf, const double* __restrict__ xs, KernelParams kp,
                                                     const double* __restrict__ a_buf, const double* __restrict__ b_buf, long a_stride,
                                                     const double* __restrict__ t_buf, long t_stride, long tile0,
                                                     double* __restrict__ out, long ldo) {
    const long I = tile0 + blockIdx.y, J = blockIdx.x;
    if (J < I) return;
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int tI = tile_leaf[I], tJ = tile_leaf[J];
    const int ancI = lv[tI].anc, ancJ = lv[tJ].anc;
    const bool same = tI == tJ;
    d4 acc = {0, 0, 0, 0};
    if (POST || !same) {
        // the lowest common ancestor: the last node of the common prefix of the two root-first chains
        const int cI = chain_ptr[tI], cJ = chain_ptr[tJ];
        const int nc = min(chain_ptr[tI + 1] - cI, chain_ptr[tJ + 1] - cJ);
        int lca = -1;
        for (int c = 0; c < nc; ++c) {
            const int i = chain[cI + c];
            if (i != chain[cJ + c]) break;
            lca = i;
        }
        int w = 0;
        if (lca >= 0) { const SiteNode N = nodes[lca]; w = N.cw + N.anc; }
        const double* xI = (POST ? b_buf : a_buf) + I * a_stride + (long)(ancI - w) * 16;
        const double* xJ = (POST ? b_buf : a_buf) + J * a_stride + (long)(ancJ - w) * 16;
        for (int k0 = 0; k0 < w; k0 += 16) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const long k = k0 + q + 4 * s;
                acc = mfma16(gld(xI + k * 16 + r), gld(xJ + k * 16 + r), acc);
            }
        }
    }
    if (same) {
        if (POST) {
            const double* aI = a_buf + I * a_stride;
            const double* aJ = a_buf + J * a_stride;
            for (int k0 = 0; k0 < ancI; k0 += 16) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const long k = k0 + q + 4 * s;
                    acc = mfma16(-gld(aI + k * 16 + r), gld(aJ + k * 16 + r), acc);
                }
            }
            const int nop = lv[tI].nop;
            const double* uI = t_buf + I * t_stride;
            const double* uJ = t_buf + J * t_stride;
            for (int k0 = 0; k0 < nop; k0 += 16) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const long k = k0 + q + 4 * s;
                    acc = mfma16(-gld(uI + k * 16 + r), gld(uJ + k * 16 + r), acc);
                }
            }
        }
        double xw[DIM];
#pragma unroll
        for (int e = 0; e < DIM; ++e) xw[e] = gld(xs + (J * 16 + r) * DIM + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double xu[DIM];
#pragma unroll
            for (int e = 0; e < DIM; ++e) xu[e] = gld(xs + (I * 16 + q + 4 * j) * DIM + e);
            acc[j] += site_cov_pair<DIM, MODE>(kp, xu, xw);
        }
    }
    double* o = out + (long)blockIdx.y * 16 * ldo + J * 16 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) gst(o + (long)(q + 4 * j) * ldo, acc[j]);
}

// ---- 6. draws at new sites (mra_sample_sites) --------------------------------------------------------------------
// Section 13's covariance is F F^T with a tree-shaped F: x(s_u) = sum over the chain of X_j(u)^T xi_j + (L_l zeta_l)_u, X = a (prior) or
// p (posterior: k_site_chain's b), L_l L_l^T = G_l = C(S_l, S_l) - a^T a [- t^T t] over the call's sites S_l of leaf l, in the caller's
// order.  A batch holds whole leaves; SiteDrawTile gives a tile its leaf's block and its place in it.
//
// A site whose leaf term is structurally zero (it lies on an ancestor's knot, so a(s) reproduces C(s, s)) is INERT: G_uu <= 2^-40 C(s, s).
// Its row and column of G_l become the identity and its zeta is not used, as k_sample_mask does for non-knot rows.  On the CPU twin
// (g32, c1, kat3, u3; 40 off-row sites and every reported row) the sites on ancestor knots had |G_uu| / C(s, s) <= 4.4e-16, the
// smallest genuine relative diagonal was 1.4e-8 and the smallest relative Cholesky pivot 1.4e-9 (c1): 2^-40 = 9.1e-13 lies between.
constexpr double SITE_INERT_REL = 0x1p-40;

// live[site] = 1 when the site is no padding column and not inert: G_uu = C(s, s) - |a|^2 [- |t|^2] in site_colsq's fixed order
template <int MODE, bool POST>
__global__ __launch_bounds__(64, 4) void k_site_inert(const SolveLeaf* __restrict__ lv, const int* __restrict__ tile_leaf, KernelParams kp,
                                                      const double* __restrict__ a_buf, long a_stride, const double* __restrict__ t_buf,
                                                      long t_stride, const long* __restrict__ sslot, int* __restrict__ live) {
    const long tile = blockIdx.x;
    const int t = tile_leaf[tile];
    const int anc = lv[t].anc, nop = lv[t].nop;
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const double c = site_cov0<MODE>(kp);
    double g = c - site_colsq(a_buf + tile * a_stride, anc, r, q);
    if (POST) g -= site_colsq(t_buf + tile * t_stride, nop, r, q);
    if (q == 0) live[tile * 16 + r] = (sslot[tile * 16 + r] >= 0 && g > SITE_INERT_REL * c) ? 1 : 0;
}

// One wave per 16 x 16 block on or below the diagonal of a leaf's G_l: tile I = blockIdx.x of the batch (M), tile J = the leaf's
// blockIdx.y-th (N).  k_site_gram's same-leaf operand pattern without p^T p (that part is the coarse term): both operands are rows of
// x16 arrays, a over anc and t over nop with the A operand negated, C(s_u, s_w) added by the lane that holds the element.  Rows and
// columns of padding and inert sites become the identity; the diagonal block is written in full.
template <int DIM, int MODE, bool POST>
__global__ __launch_bounds__(64, 4) void k_site_leaf_gram(const SolveLeaf* __restrict__ lv, const int* __restrict__ tile_leaf,
                                                          const SiteDrawTile* __restrict__ dt, const double* __restrict__ xs, KernelParams kp,
                                                          const double* __restrict__ a_buf, long a_stride, const double* __restrict__ t_buf,
                                                          long t_stride, const int* __restrict__ live, double* __restrict__ G) {
    const long I = blockIdx.x;
    const SiteDrawTile D = dt[I];
    const int il = (int)(I - D.first), jl = blockIdx.y;
    if (jl > il) return;
    const long J = (long)D.first + jl;
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int t = tile_leaf[I];
    const int anc = lv[t].anc;
    d4 acc = {0, 0, 0, 0};
    const double* aI = a_buf + I * a_stride;
    const double* aJ = a_buf + J * a_stride;
    for (int k0 = 0; k0 < anc; k0 += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long k = k0 + q + 4 * s;
            acc = mfma16(-gld(aI + k * 16 + r), gld(aJ + k * 16 + r), acc);
        }
    }
    if (POST) {
        const int nop = lv[t].nop;
        const double* uI = t_buf + I * t_stride;
        const double* uJ = t_buf + J * t_stride;
        for (int k0 = 0; k0 < nop; k0 += 16) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const long k = k0 + q + 4 * s;
                acc = mfma16(-gld(uI + k * 16 + r), gld(uJ + k * 16 + r), acc);
            }
        }
    }
    double xw[DIM];
#pragma unroll
    for (int e = 0; e < DIM; ++e) xw[e] = gld(xs + (J * 16 + r) * DIM + e);
    const int lw = live[J * 16 + r];
    const long ld = 16L * D.nt;
    double* o = G + D.goff + (long)il * 16 * ld + jl * 16 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double xu[DIM];
#pragma unroll
        for (int e = 0; e < DIM; ++e) xu[e] = gld(xs + (I * 16 + q + 4 * j) * DIM + e);
        const double v = acc[j] + site_cov_pair<DIM, MODE>(kp, xu, xw);
        const bool both = lw && live[I * 16 + q + 4 * j];
        gst(o + (long)(q + 4 * j) * ld, both ? v : ((il == jl && q + 4 * j == r) ? 1.0 : 0.0));
    }
}

// the leaf draws of a block of 16 samples, staged once per leaf: zl[site * 16 + s] = zeta of the site's own slot n_coarse + (the
// caller's index of the site) - Philox exactly as k_sample_draw, or the caller's value (zin, same layout) - and 0 for padding sites,
// inert sites and samples past the block's count
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(256) void k_site_zeta(SampleZ zs, long n_coarse, const long* __restrict__ sslot, const int* __restrict__ live,
                                                   const double* __restrict__ zin, long n_sites, double* __restrict__ zl) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sites * 16) return;
    const long u = i >> 4;
    const int s = (int)(i & 15);
    double v = 0.0;
    if (live[u] && s < zs.ns)
        v = zin ? gld(zin + i) : philox_normal(zs.seed, (unsigned long long)(n_coarse + sslot[u]), (unsigned long long)(zs.sample0 + s));
    zl[i] = v;
}
#endif

// One wave per (tile, block of 16 samples): the 16 sites are M, the samples N; lane (r, q) leaves (site q + 4 j, sample r).
//   coarse term  over the leaf's chain: X[rows of block j]^T zc[slots of j] - X in x16 form (the A operand of k-step s is row k of X at
//                lane r), zc slot-major as k_sample_coarse reads it
//   leaf term    L_l[tile rows, 0 .. tile end] zeta_l: L_l row-major in the leaf's block, the entries above the diagonal inside the
//                diagonal tile masked (k_panel_chol leaves that part of the block as it was)
//   mean         the posterior mean of the plan's own observations (k_site_mean's column 0), added last; nullptr: none
// out[sample * ldo + tile * 16 + site].
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(64, 4) void k_site_draw(const int* __restrict__ tile_leaf, const SiteDrawTile* __restrict__ dt,
                                                     const int* __restrict__ dchain_ptr, const SiteDrawChain* __restrict__ dchain,
                                                     const double* __restrict__ x_buf, long a_stride, const double* __restrict__ zc,
                                                     const double* __restrict__ G, const double* __restrict__ zl,
                                                     const double* __restrict__ mean, double* __restrict__ out, long ldo) {
    const long tile = blockIdx.x;
    const int t = tile_leaf[tile];
    const SiteDrawTile D = dt[tile];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    d4 acc = {0, 0, 0, 0};
    const double* X = x_buf + tile * a_stride;
    const int e1 = dchain_ptr[t + 1];
    for (int e = dchain_ptr[t]; e < e1; ++e) {
        const SiteDrawChain c = dchain[e];
        const double* xp = X + (long)c.row * 16 + r;
        const double* zp = zc + (long)c.zoff * 16 + r;
        for (int k0 = 0; k0 < c.width; k0 += 16) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const long k = k0 + q + 4 * s;
                acc = mfma16(gld(xp + k * 16), gld(zp + k * 16), acc);
            }
        }
    }
    const int il = (int)(tile - D.first);
    const long ld = 16L * D.nt;
    const double* Lrow = G + D.goff + ((long)il * 16 + r) * ld;
    const double* zt = zl + (long)D.first * 256 + r;
    for (int J = 0; J <= il; ++J) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = q + 4 * s;
            const double l = gld(Lrow + J * 16 + k);
            acc = mfma16((J == il && k > r) ? 0.0 : l, gld(zt + (long)(J * 16 + k) * 16), acc);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long u = tile * 16 + q + 4 * j;
        gst(out + (long)r * ldo + u, mean ? acc[j] + gld(mean + u) : acc[j]);
    }
}
#endif

// ---- 7. cross-validation from the retained factors (mra_cv) -----------------------------------------------------
// The sites are the plan's own observed rows, tiled by leaf: sslot[tile * 16 + k] = the padded row of the column (-1: padding).  After the
// four site kernels above a tile holds a, t, p (k_site_chain's b), the posterior variance v and the posterior mean m of its rows.  With
// D = diag(r) the noise, rho = y - m and N_G = D_G - Sigma_post[G, G] for a group G of observed rows, the predictive distribution of y_G
// given every observation outside G has mean y_G - D_G N_G^-1 rho_G and covariance D_G N_G^-1 D_G (noise included).  The information sits
// in r - v: with h = v / r float64 loses about eps / (1 - h)^2, whatever computes it.
constexpr double CV_LOG_2PI = 1.8378770664093454836;
static const int CV_BLOCKS = 1024;          // partial results of the reduction: a fixed number, folded in a fixed order (as k_laplace_part)

__device__ __forceinline__ double cv_noise(const CvRows& c, long p) { return c.noise ? c.noise[p] : c.R; }

// the coordinates of a batch's sites out of the plan's rows; padding columns repeat their tile's first site (as sites_gather)
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(256) void k_cv_sites(const long* __restrict__ sslot, const double* __restrict__ X, int d, long n_sites,
                                                  double* __restrict__ xs) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sites) return;
    long p = sslot[i];
    if (p < 0) p = sslot[i & ~15L];
    for (int k = 0; k < d; ++k) xs[i * d + k] = X[p * d + k];
}
#endif

// leave one out: every observed row its own group, so N_G = r (1 - h).  1 - h <= 0 or NaN: err = the largest such padded row + 1.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(256) void k_cv_loo(const long* __restrict__ sslot, long n_sites, const double* __restrict__ v,
                                                const double* __restrict__ m, CvRows c, CvOut o, int* __restrict__ err) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sites) return;
    const long p = sslot[i];
    if (p < 0) return;
    const double r = cv_noise(c, p), y = c.y[p], h = v[i] / r, om = 1.0 - h, rho = y - m[i];
    if (!(om > 0.0)) atomicMax(err, (int)(p + 1));
    const double e = rho / om, S = r / om;
    o.mean[p] = y - e; o.var[p] = S; o.lpd[p] = -0.5 * (CV_LOG_2PI + log(S) + e * e / S);
    o.h[p] = h; o.rho[p] = rho;
}
#endif

// One wave per 16 x 16 block on or below the diagonal of a leaf's N_G = diag(r) - [p^T p - a^T a - t^T t + C(s_u, s_w)]: tile I =
// blockIdx.x of the batch (M), tile J = the leaf's blockIdx.y-th (N).  k_site_leaf_gram's operand pattern (both operands rows of x16
// arrays, the covariance added by the lane that holds the element) plus k_site_gram's p^T p over the whole chain, which is all of anc.
// Rows and columns of padding become the identity.
template <int DIM, int MODE>
__global__ __launch_bounds__(64, 4) void k_cv_gram(const SolveLeaf* __restrict__ lv, const int* __restrict__ tile_leaf,
                                                   const SiteDrawTile* __restrict__ dt, const double* __restrict__ xs, KernelParams kp,
                                                   const double* __restrict__ a_buf, const double* __restrict__ b_buf, long a_stride,
                                                   const double* __restrict__ t_buf, long t_stride, const long* __restrict__ sslot,
                                                   CvRows c, double* __restrict__ G) {
    const long I = blockIdx.x;
    const SiteDrawTile D = dt[I];
    const int il = (int)(I - D.first), jl = blockIdx.y;
    if (jl > il) return;
    const long J = (long)D.first + jl;
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int t = tile_leaf[I];
    const int anc = lv[t].anc, nop = lv[t].nop;
    d4 acc = {0, 0, 0, 0};
    const double* pI = b_buf + I * a_stride;
    const double* pJ = b_buf + J * a_stride;
    const double* aI = a_buf + I * a_stride;
    const double* aJ = a_buf + J * a_stride;
    for (int k0 = 0; k0 < anc; k0 += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long k = k0 + q + 4 * s;
            acc = mfma16(-gld(pI + k * 16 + r), gld(pJ + k * 16 + r), acc);
        }
    }
    for (int k0 = 0; k0 < anc; k0 += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long k = k0 + q + 4 * s;
            acc = mfma16(gld(aI + k * 16 + r), gld(aJ + k * 16 + r), acc);
        }
    }
    const double* uI = t_buf + I * t_stride;
    const double* uJ = t_buf + J * t_stride;
    for (int k0 = 0; k0 < nop; k0 += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const long k = k0 + q + 4 * s;
            acc = mfma16(gld(uI + k * 16 + r), gld(uJ + k * 16 + r), acc);
        }
    }
    double xw[DIM];
#pragma unroll
    for (int e = 0; e < DIM; ++e) xw[e] = gld(xs + (J * 16 + r) * DIM + e);
    const bool lw = sslot[J * 16 + r] >= 0;
    const long ld = 16L * D.nt;
    double* o = G + D.goff + (long)il * 16 * ld + jl * 16 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double xu[DIM];
#pragma unroll
        for (int e = 0; e < DIM; ++e) xu[e] = gld(xs + (I * 16 + q + 4 * j) * DIM + e);
        const long pu = sslot[I * 16 + q + 4 * j];
        const bool on_diag = il == jl && q + 4 * j == r;
        double v = acc[j] - site_cov_pair<DIM, MODE>(kp, xu, xw);
        if (on_diag && pu >= 0) v += cv_noise(c, pu);
        gst(o + (long)(q + 4 * j) * ld, (lw && pu >= 0) ? v : (on_diag ? 1.0 : 0.0));
    }
}

// One wave per group, after k_panel_chol left N_G = L L^T in the group's block: w = L^-1 rho_G in column 0 of an x16 array (the other
// columns are zero), and the group's joint log predictive density -1/2 [2 sum log r - log det N_G + |w|^2 + |G| log 2 pi] at its node.
// dn: k_panel_chol's 2 sum log diag L per group of the batch (padding rows are the identity and add 0).
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(64, 4) void k_cv_fwd(const CvGroup* __restrict__ groups, const long* __restrict__ sslot,
                                                  const double* __restrict__ m, CvRows c, const double* __restrict__ G,
                                                  const double* __restrict__ dn, double* __restrict__ w_buf, double* __restrict__ group_lpd) {
    __shared__ double Ld[256];
    const CvGroup g = groups[blockIdx.x];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    double* w = w_buf + (long)g.first * 256;
    site_trsm(G + g.goff, 16 * g.nt, g.nt, w, Ld, [&](int I) {
        d4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long u = ((long)g.first + I) * 16 + q + 4 * j;
            const long p = sslot[u];
            acc[j] = (r == 0 && p >= 0) ? c.y[p] - m[u] : 0.0;
        }
        return acc;
    });
    const double quad = __shfl(site_colsq(w, 16 * g.nt, r, q), 0, 64);
    double s = 0.0, cnt = 0.0;
    for (int u = lane; u < 16 * g.nt; u += 64) {
        const long p = sslot[(long)g.first * 16 + u];
        if (p >= 0) { s += log(cv_noise(c, p)); cnt += 1.0; }
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) { s += __shfl_xor(s, k, 64); cnt += __shfl_xor(cnt, k, 64); }
    if (lane == 0) group_lpd[g.node] = -0.5 * (2.0 * s - dn[blockIdx.x] + quad + cnt * CV_LOG_2PI);
}
#endif

// One wave per (group, column tile c): X_c = L^-1 E_c by forward substitution (its rows above tile c are zero and are not computed: the
// trailing block of L is solved), then for the tile's rows diag(N^-1)_p = the column sums of squares of X_c and (N^-1 rho)_p = X_c[:, p]^T w
// - N^-1 = L^-T L^-1, so no backward substitution is run.  y_p - mu_p = r_p (N^-1 rho)_p, S_pp = r_p^2 diag(N^-1)_p.
// x_buf: the batch's second block buffer, tile c of a group using the rows of the group's block from its own first row on.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(64, 4) void k_cv_solve(const SiteDrawTile* __restrict__ dt, const long* __restrict__ sslot,
                                                    const double* __restrict__ v, const double* __restrict__ m, CvRows c,
                                                    const double* __restrict__ G, const double* __restrict__ w_buf,
                                                    double* __restrict__ x_buf, CvOut o) {
    __shared__ double Ld[256];
    const long I = blockIdx.x;
    const SiteDrawTile D = dt[I];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int cI = (int)(I - D.first), nt = D.nt - cI;
    const long ld = 16L * D.nt;
    double* x = x_buf + D.goff + (long)cI * 16 * ld;
    site_trsm(G + D.goff + (long)cI * 16 * ld + cI * 16, (int)ld, nt, x, Ld, [&](int K) {
        d4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = (K == 0 && q + 4 * j == r) ? 1.0 : 0.0;
        return acc;
    });
    const double dg = site_colsq(x, 16 * nt, r, q);
    const double* w = w_buf + I * 256;
    double dot = 0.0;
    for (int k = q; k < 16 * nt; k += 4) dot = __builtin_fma(gld(x + (long)k * 16 + r), gld(w + (long)k * 16), dot);
    dot += __shfl_xor(dot, 16, 64);
    dot += __shfl_xor(dot, 32, 64);
    const long u = I * 16 + r;
    const long p = sslot[u];
    if (q == 0 && p >= 0) {
        const double rr = cv_noise(c, p), y = c.y[p], e = rr * dot, S = rr * rr * dg;
        o.mean[p] = y - e; o.var[p] = S; o.lpd[p] = -0.5 * (CV_LOG_2PI + log(S) + e * e / S);
        o.h[p] = v[u] / rr; o.rho[p] = y - m[u];
    }
}
#endif

// leave one out: a leaf's group value is the sum of its rows' lpd, in row order (one thread per leaf); NaN for a leaf without observations
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(256) void k_cv_leaf_sum(const int* __restrict__ leaf_node, const long* __restrict__ leaf_row, int n_leaves,
                                                     const double* __restrict__ lpd, double* __restrict__ group_lpd) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_leaves) return;
    double s = 0.0;
    bool any = false;
    for (long p = leaf_row[2 * t]; p < leaf_row[2 * t + 1]; ++p) {
        const double l = lpd[p];
        if (l == l) { s += l; any = true; }
    }
    if (any) group_lpd[leaf_node[t]] = s;
}
#endif

// Per workgroup {rows, sum lpd, sum (y - mu)^2 / S, max h, sum (1 - h) / r, sum (rho / r)^2, sum of the groups' values}: a thread walks
// its rows (then its nodes) in order, the workgroup folds its 256 values in a fixed tree, as k_laplace_part: the same inputs give the
// same bits.  A row counts when it was scored (h is not NaN), a node when its group value is not NaN.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(256) void k_cv_part(CvRows c, CvOut o, long P, const double* __restrict__ group_lpd, int n_nodes,
                                                 double* __restrict__ part) {
    __shared__ double sh[MRA_CV_NRES][256];
    double a[MRA_CV_NRES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
        const double h = o.h[p];
        if (!(h == h)) continue;
        const double r = cv_noise(c, p), e = c.y[p] - o.mean[p], al = o.rho[p] / r;
        a[0] += 1.0;
        a[1] += o.lpd[p];
        a[2] += e * e / o.var[p];
        a[3] = h > a[3] ? h : a[3];
        a[4] += (1.0 - h) / r;
        a[5] += al * al;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_nodes; i += gridDim.x * 256) {
        const double l = group_lpd[i];
        if (l == l) a[6] += l;
    }
#pragma unroll
    for (int k = 0; k < MRA_CV_NRES; ++k) sh[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < MRA_CV_NRES; ++k) {
                const double x = sh[k][threadIdx.x], y = sh[k][threadIdx.x + w];
                sh[k][threadIdx.x] = k == 3 ? (y > x ? y : x) : x + y;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < MRA_CV_NRES) part[(long)blockIdx.x * MRA_CV_NRES + threadIdx.x] = sh[threadIdx.x][0];
}
#endif
// the workgroups' partial results -> res[MRA_CV_NRES]: one wave per result, as k_laplace_sum
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(64 * MRA_CV_NRES) void k_cv_sum(const double* __restrict__ part, int nblk, double* __restrict__ res) {
    __shared__ double sh[MRA_CV_NRES][64];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int b = lane; b < nblk; b += 64) {
        const double a = part[(long)b * MRA_CV_NRES + k];
        acc = k == 3 ? (a > acc ? a : acc) : acc + a;
    }
    sh[k][lane] = acc;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if (lane < w) {
            const double a = sh[k][lane], b = sh[k][lane + w];
            sh[k][lane] = k == 3 ? (b > a ? b : a) : a + b;
        }
        __syncthreads();
    }
    if (lane == 0) res[k] = sh[k][0];
}
#endif

// ---- 8. cross-validation with a regression trend (mra_cv_trend) -------------------------------------------------
// y = X beta + x + eps with a flat prior on beta.  After mra_trend_fit's sweeps trend.m holds the kriging means of [y | X], trend.coef
// beta^ and L_A^-1 (A = X^T K^-1 X = L_A L_A^T).  With h_p = X_p - m_X(p) and w_p = L_A^-1 h_p: K^-1 X = D^-1 h, P y = D^-1 rho~ with
// rho~_p = y_p - m_y(p) - h_p^T beta^, and P[G, G] = D_G^-1 (N_G - W_G W_G^T) D_G^-1.  So section 18's formulas hold with rho~ for rho
// and, when beta is estimated again without the group, N_G - W_G W_G^T for N_G (by row: h~ = (v + |w|^2) / r for h).
//
// One wave per tile, after k_site_mean: h for the tile's rows out of X and m_X (lane (r, q) loads row r's covariates q, q + 4, ...: for
// one covariate 16 neighbouring rows), W^T = L_A^-1 h^T (qn x16, qn = p rounded up to 4) block row by block row on the MFMA - L_A^-1
// comes out of L2, 32 KB for all tiles, and only its lower triangle is read - then |w|^2 per row and m[u] += h^T beta^ (the sum in
// k_trend_rows' order), so that k_cv_loo, k_cv_fwd and k_cv_solve see rho~ = y - m.  add_v: v[u] += |w|^2 as well, which makes
// k_cv_loo's h the h~ of leaving a row out and estimating beta again.  Padding columns get w = 0 and keep their m and v.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(64, 4) void k_cv_trend(const long* __restrict__ sslot, const double* __restrict__ X, const double* __restrict__ mX,
                                                    long P, int p, const double* __restrict__ beta, const double* __restrict__ Linv,
                                                    int add_v, double* __restrict__ m, double* __restrict__ v, double* __restrict__ w_buf,
                                                    double* __restrict__ wsq) {
    const long I = blockIdx.x;
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int qn = (p + 3) & ~3, nb = (p + 15) >> 4;
    const long u = I * 16 + r;
    const long row = sslot[u];
    // h[s] = h_row[q + 4 s]: the B operand of every k-step, and the terms of h^T beta^
    double h[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int j = q + 4 * s;
        h[s] = (row >= 0 && j < p) ? gld(X + (long)j * P + row) - gld(mX + (long)j * P + row) : 0.0;
    }
    double* w = w_buf + I * (long)qn * 16;
    double sq = 0.0;
#pragma unroll
    for (int B = 0; B < 4; ++B) {
        if (B < nb) {                            // (uniform: the unrolled loops keep h in registers)
            d4 acc = {0, 0, 0, 0};
            const int i = B * 16 + r;            // the row of L_A^-1 this lane feeds
#pragma unroll
            for (int J = 0; J <= B; ++J) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = J * 16 + q + 4 * s;
                    if (J * 16 + 4 * s < qn) {
                        const double a = (k <= i && i < p) ? gld(Linv + (long)i * (MRA_TREND_MAX + 1) + k) : 0.0;
                        acc = mfma16(a, h[J * 4 + s], acc);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int wi = B * 16 + q + 4 * j;
                if (wi < qn) gst(w + (long)wi * 16 + r, acc[j]);
                sq = __builtin_fma(acc[j], acc[j], sq);
            }
        }
    }
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    // h^T beta^ for row r, one covariate after the other as k_trend_rows sums them (covariate j sits in lane (r, j & 3), element j >> 2)
    double mu = gld(m + u);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double hj = __shfl(h[s], r + 16 * k, 64);
            if (4 * s + k < p) mu = __builtin_fma(hj, beta[4 * s + k], mu);
        }
    }
    if (q == 0 && row >= 0) {
        gst(m + u, mu);
        if (add_v) gst(v + u, gld(v + u) + sq);
        wsq[row] = sq;
    }
}
#endif

// One wave per 16 x 16 block on or below the diagonal of a leaf's block, k_cv_gram's grid and operand pattern: N -= W_I W_J^T over the
// qn = p rounded up to 4 rows of the tiles' W arrays, qn / 4 MFMAs.  Padding rows and columns have w = 0 and stay the identity.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(64, 4) void k_cv_downdate(const SiteDrawTile* __restrict__ dt, const double* __restrict__ w_buf, int qn,
                                                       double* __restrict__ G) {
    const long I = blockIdx.x;
    const SiteDrawTile D = dt[I];
    const int il = (int)(I - D.first), jl = blockIdx.y;
    if (jl > il) return;
    const long J = (long)D.first + jl;
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const long ld = 16L * D.nt;
    double* o = G + D.goff + (long)il * 16 * ld + jl * 16 + r;
    d4 acc;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = gld(o + (long)(q + 4 * j) * ld);
    const double* wI = w_buf + I * (long)qn * 16;
    const double* wJ = w_buf + J * (long)qn * 16;
    for (int k0 = 0; k0 < qn; k0 += 4) {
        const long k = k0 + q;
        acc = mfma16(-gld(wI + k * 16 + r), gld(wJ + k * 16 + r), acc);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) gst(o + (long)(q + 4 * j) * ld, acc[j]);
}
#endif

// The trend's share of the reduction, in the pattern of k_cv_part / k_cv_sum: per workgroup {tr K^-1 = sum (1 - v / r) / r,
// tr P = sum (1 - (v + |w|^2) / r) / r, max (v + |w|^2) / r} over the scored rows.  h_has_w: the rows' h is h~ already (k_cv_trend added
// |w|^2 to v), else it is v / r.
constexpr int MRA_CVT_NRES = 3;
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_sites.hip */
__global__ __launch_bounds__(256) void k_cv_trend_part(CvRows c, CvOut o, const double* __restrict__ wsq, int h_has_w, long P,
                                                       double* __restrict__ part) {
    __shared__ double sh[MRA_CVT_NRES][256];
    double a[MRA_CVT_NRES] = {0.0, 0.0, 0.0};
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
        const double h = o.h[p];
        if (!(h == h)) continue;
        const double r = cv_noise(c, p), dw = wsq[p] / r;
        const double hv = h_has_w ? h - dw : h, ht = h_has_w ? h : h + dw;
        a[0] += (1.0 - hv) / r;
        a[1] += (1.0 - ht) / r;
        a[2] = ht > a[2] ? ht : a[2];
    }
#pragma unroll
    for (int k = 0; k < MRA_CVT_NRES; ++k) sh[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < MRA_CVT_NRES; ++k) {
                const double x = sh[k][threadIdx.x], y = sh[k][threadIdx.x + w];
                sh[k][threadIdx.x] = k == 2 ? (y > x ? y : x) : x + y;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < MRA_CVT_NRES) part[(long)blockIdx.x * MRA_CVT_NRES + threadIdx.x] = sh[threadIdx.x][0];
}
__global__ __launch_bounds__(64 * MRA_CVT_NRES) void k_cv_trend_sum(const double* __restrict__ part, int nblk, double* __restrict__ res) {
    __shared__ double sh[MRA_CVT_NRES][64];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int b = lane; b < nblk; b += 64) {
        const double a = part[(long)b * MRA_CVT_NRES + k];
        acc = k == 2 ? (a > acc ? a : acc) : acc + a;
    }
    sh[k][lane] = acc;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if (lane < w) {
            const double a = sh[k][lane], b = sh[k][lane + w];
            sh[k][lane] = k == 2 ? (b > a ? b : a) : a + b;
        }
        __syncthreads();
    }
    if (lane == 0) res[k] = sh[k][0];
}
#endif
