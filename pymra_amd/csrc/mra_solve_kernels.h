// mra_solve_kernels.h - kernels of mra_solve: the factors a likelihood pass leaves in the plan (the leaves'
// L_c and Ut, the fronts' Lt and Zt, the prior W) used as a sparse direct solver for a block of 16 right-hand sides.  Included by
// mra_launch_solve.hip only, so that the other translation units keep their object code.
//
// All 16-column work arrays are row-major with 16 doubles per row ("x16"): element (row, column) at row * 16 + column.  Columns
// >= n_cols of a block hold zeros on input and are computed as zeros, not branched around.
// MFMA conventions (mra_kernels.h): lane (r, q) = (lane & 15, lane >> 4); mfma16(a, b, acc) over k-step s takes a = A[r][q + 4 s],
// b = B[q + 4 s][r] and leaves D[q + 4 j][r] in acc[j].
#pragma once
#include "mra_plan_types.h"      // SolveLeaf, SolveFront, SolveSeg; mra_kernels.h

// ---- leaves: triangular solves with L_c, one wave per leaf ---------------------------------------------------------------------
// Forward (BACK = false): uy = L_c^-1 Y[obs, 0:16], Y read from the 16 x P block Yb at the observed rows.  Backward (BACK = true):
// uy <- L_c^-T uy in place.  Off-diagonal tiles on the MFMA; the 16 x 16 diagonal block by substitution across the wave (the block
// in LDS, the solved row broadcast with one shuffle per step).
template <bool BACK>
__global__ __launch_bounds__(64, 4) void k_solve_leaf_trsm(const SolveLeaf* __restrict__ lv, const double* __restrict__ Yb, long P) {
    const SolveLeaf L = lv[blockIdx.x];
    const int nop = L.nop, nt = nop >> 4;
    if (!nt) return;
    __shared__ double Ld[256];
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    for (int step = 0; step < nt; ++step) {
        const int I = BACK ? nt - 1 - step : step;
        d4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = I * 16 + q + 4 * j;
            if (BACK) acc[j] = gld(L.uy + (long)k * 16 + r);
            else {
                const int o = gldi(L.obs + k);
                acc[j] = o >= 0 ? gld(Yb + (long)r * P + o) : 0.0;
            }
        }
        for (int J = BACK ? I + 1 : 0; J < (BACK ? nt : I); ++J) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = J * 16 + q + 4 * s;
                // forward: A = L[I][J]; backward: A = L[J][I]^T
                const double a = BACK ? gld(L.Lc + (long)k * nop + I * 16 + r) : gld(L.Lc + (long)(I * 16 + r) * nop + k);
                acc = mfma16(-a, gld(L.uy + (long)k * 16 + r), acc);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) Ld[lane + 64 * j] = gld(L.Lc + (long)(I * 16 + (lane >> 4) + 4 * j) * nop + I * 16 + (lane & 15));
        __syncthreads();
        // Ld[i * 16 + k] = L_II[i][k]; lane (r, q) holds rows q + 4 j of column r
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const int k = BACK ? 15 - kk : kk;
            const double xk = __shfl(acc[k >> 2], r + 16 * (k & 3), 64) / Ld[k * 17];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = q + 4 * j;
                const double l = BACK ? Ld[k * 16 + row] : Ld[row * 16 + k];
                if (BACK ? row < k : row > k) acc[j] = __builtin_fma(-l, xk, acc[j]);
                if (row == k) acc[j] = xk;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) gst(L.uy + (long)(I * 16 + q + 4 * j) * 16 + r, acc[j]);
        __syncthreads();             // the tile is read back by every lane of the wave in the next steps
    }
}

// ---- leaves: products with Ut, one workgroup of four waves per leaf ------------------------------------------------------------
// Forward: g = Ut_anc U_y (anc x16).
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256, 4) void k_solve_leaf_g(const SolveLeaf* __restrict__ lv) {
    const SolveLeaf L = lv[blockIdx.x];
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4, nop = L.nop;
    for (int at = threadIdx.x >> 6; at < (L.anc >> 4); at += 4) {
        d4 acc = {0, 0, 0, 0};
        for (int o0 = 0; o0 < nop; o0 += 16) {
            const d4 a = load_rowlane(L.Ut + (long)at * 16 * nop + o0, nop, r, q);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma16(a[s], gld(L.uy + (long)(o0 + q + 4 * s) * 16 + r), acc);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) gst(L.gb + (long)(at * 16 + q + 4 * j) * 16 + r, acc[j]);
    }
}
#endif

// Backward: s = U_y - Ut_anc^T alpha_chain in place (nop x16; phantom observations stay 0), then beta = alpha_chain - Ut_anc s
// (anc x16, over g).  A leaf without observations has beta = alpha_chain.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256, 4) void k_solve_leaf_sbeta(const SolveLeaf* __restrict__ lv) {
    const SolveLeaf L = lv[blockIdx.x];
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4, nop = L.nop, w = threadIdx.x >> 6;
    for (int ot = w; ot < (nop >> 4); ot += 4) {
        d4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = gld(L.uy + (long)(ot * 16 + q + 4 * j) * 16 + r);
        for (int a0 = 0; a0 < L.anc; a0 += 16) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int a = a0 + q + 4 * s;
                acc = mfma16(-gld(L.Ut + (long)a * nop + ot * 16 + r), gld(L.chain + (long)a * 16 + r), acc);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = ot * 16 + q + 4 * j;
            gst(L.uy + (long)k * 16 + r, gldi(L.obs + k) >= 0 ? acc[j] : 0.0);
        }
    }
    __syncthreads();
    for (int at = w; at < (L.anc >> 4); at += 4) {
        d4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = gld(L.chain + (long)(at * 16 + q + 4 * j) * 16 + r);
        for (int o0 = 0; o0 < nop; o0 += 16) {
            const d4 a = load_rowlane(L.Ut + (long)at * 16 * nop + o0, nop, r, q);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma16(-a[s], gld(L.uy + (long)(o0 + q + 4 * s) * 16 + r), acc);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) gst(L.gb + (long)(at * 16 + q + 4 * j) * 16 + r, acc[j]);
    }
}
#endif

// ---- fronts: one workgroup per node, one launch per level (latency kernels, like k_front) ---------------------------------------
// cw x16 substitution by wave 0: lane (c, q) sums the terms j = q (mod 4) of a row, two shuffles add the four partial sums.
// Ls: Lt staged in LDS (cw x cw, blocks of at most SOLVE_FRONT_STAGE columns), or nullptr: read from F.
#define SOLVE_FRONT_STAGE 64
__device__ __forceinline__ double solve_lt(const double* __restrict__ F, int ld, const double* Ls, int cw, int i, int j) {
    return Ls ? Ls[i * cw + j] : gld(F + (long)i * ld + j);
}
__device__ __forceinline__ const double* solve_front_stage(const double* __restrict__ F, int ld, int cw, double* Ls) {
    if (cw > SOLVE_FRONT_STAGE) return nullptr;
    for (int e = threadIdx.x; e < cw * cw; e += 256) Ls[e] = gld(F + (long)(e / cw) * ld + e % cw);
    return Ls;
}
__device__ __forceinline__ void solve_front_subst(const double* __restrict__ F, int ld, const double* Ls, int cw, volatile double* zs, bool back) {
    const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
    for (int kk = 0; kk < cw; ++kk) {
        const int k = back ? cw - 1 - kk : kk;
        double part = 0.0;
        if (back) { for (int j = k + 1 + q; j < cw; j += 4) part = __builtin_fma(solve_lt(F, ld, Ls, cw, j, k), zs[j * 16 + c], part); }
        else      { for (int j = q; j < k; j += 4) part = __builtin_fma(solve_lt(F, ld, Ls, cw, k, j), zs[j * 16 + c], part); }
        part += __shfl_xor(part, 16, 64);
        part += __shfl_xor(part, 32, 64);
        const double x = (zs[k * 16 + c] - part) / solve_lt(F, ld, Ls, cw, k, k);
        if (q == 0) zs[k * 16 + c] = x;
        __builtin_amdgcn_wave_barrier();
    }
}

// Forward: f = sum over the children's g; z = Lt^-1 f[own]; g = f[anc] - Zt z.  buf <- [z ; g].
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256) void k_solve_front_fwd(const SolveFront* __restrict__ fv, const double* const* __restrict__ kids) {
    extern __shared__ double zs[];              // cw x16, then Lt when it is staged
    const SolveFront N = fv[blockIdx.x];
    const int nown = N.cw * 16, nall = (N.cw + N.anc) * 16;
    const double* Ls = solve_front_stage(N.F, N.ld, N.cw, zs + nown);
    for (int e = threadIdx.x; e < nall; e += 256) {
        double f = 0.0;
        for (int k = 0; k < N.nkid; ++k) f += gld(kids[N.kid0 + k] + e);
        if (e < nown) zs[e] = f; else gst(N.buf + e, f);
    }
    __syncthreads();
    if (threadIdx.x < 64) solve_front_subst(N.F, N.ld, Ls, N.cw, zs, false);
    __syncthreads();
    for (int e = threadIdx.x; e < nall; e += 256) {
        if (e < nown) { gst(N.buf + e, zs[e]); continue; }
        const int a = (e >> 4) - N.cw, c = e & 15;
        const double* zt = N.F + (long)(N.cw + a) * N.ld;
        double f = gld(N.buf + e);
        for (int k = 0; k < N.cw; ++k) f = __builtin_fma(-gld(zt + k), zs[k * 16 + c], f);
        gst(N.buf + e, f);
    }
}
#endif

// Backward: alpha = Lt^-T (z - Zt^T alpha_chain).  buf <- [alpha ; alpha_chain].
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256) void k_solve_front_bwd(const SolveFront* __restrict__ fv) {
    extern __shared__ double zs[];
    const SolveFront N = fv[blockIdx.x];
    const int nown = N.cw * 16, nall = (N.cw + N.anc) * 16;
    const double* Ls = solve_front_stage(N.F, N.ld, N.cw, zs + nown);
    for (int e = threadIdx.x; e < nown; e += 256) {
        const int k = e >> 4, c = e & 15;
        double f = gld(N.buf + e);
        for (int a = 0; a < N.anc; ++a) f = __builtin_fma(-gld(N.F + (long)(N.cw + a) * N.ld + k), gld(N.chain + (long)a * 16 + c), f);
        zs[e] = f;
    }
    __syncthreads();
    if (threadIdx.x < 64) solve_front_subst(N.F, N.ld, Ls, N.cw, zs, true);
    __syncthreads();
    for (int e = threadIdx.x; e < nall; e += 256) gst(N.buf + e, e < nown ? zs[e] : gld(N.chain + (e - nown)));
}
#endif

// ---- quadratic form: Q = sum over segments of sign * V^T V (V: n x16), fixed summation order ------------------------------------
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256) void k_solve_quad_part(const SolveSeg* __restrict__ segs, int nseg, double* __restrict__ part) {
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    double acc = 0.0;
    for (int sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
        const SolveSeg S = segs[sgi];
        double a = 0.0;
        for (int k = 0; k < S.n; ++k) a = __builtin_fma(gld(S.p + (long)k * 16 + i), gld(S.p + (long)k * 16 + j), a);
        acc += S.sign * a;
    }
    part[(long)blockIdx.x * 256 + threadIdx.x] = acc;
}
__global__ __launch_bounds__(256) void k_solve_quad_sum(const double* __restrict__ part, int nblk, double* __restrict__ quad) {
    double acc = 0.0;
    for (int b = 0; b < nblk; ++b) acc += part[(long)b * 256 + threadIdx.x];
    quad[threadIdx.x] = acc;
}
#endif

// ---- full quadratic form (MRA_SOLVE_FULL_QUAD): the entries between columns of different 16-column blocks ------------------------
// The forward vectors of a block (every segment's n x16 rows: the leaves' U_y, the fronts' z) are copied into the block's panel of the
// archive behind its forward sweep, segment sgi at row seg_off[sgi]; one workgroup per segment, the tail of the grid strides on.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256) void k_solve_archive(const SolveSeg* __restrict__ segs, const long* __restrict__ seg_off, int nseg,
                                                       double* __restrict__ panel) {
    for (int sgi = blockIdx.x; sgi < nseg; sgi += gridDim.x) {
        const SolveSeg S = segs[sgi];
        double* dst = panel + seg_off[sgi] * 16;
        for (int e = threadIdx.x; e < S.n * 16; e += 256) gst(dst + e, gld(S.p + e));
    }
}
#endif

// Q_ab = sum over segments of sign * F_a^T F_b for the block pairs of one group: four panels u < v of the archive, their six pairs
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) accumulated side by side so that a row of the archive is read once per launch.  blk[u] < 0: the
// slot is empty (its rows are not read); out[p]: whether pair p is wanted (a pair of an earlier group, or one with an empty slot, is not).
struct QuadGroup { int blk[4]; int out[6]; };
// The A operand of v_mfma_f64_16x16x4_f64 is four rows of panel a, transposed, the B operand the same four rows of panel b: lane
// (i, kk) = (lane & 15, lane >> 4) loads F[k0 + kk][i] of either - a wave's load is 4 rows x 16 doubles, 512 contiguous bytes - and
// acc[j] is Q_ab[kk + 4 j][i].  The sign goes onto the A operand (exact).  Rows past a segment's n are not read (a masked tail: the
// operands of those lanes are 0).  The segments are dealt to the workgroups as k_solve_quad_part deals them, a segment's 4-row chunks
// to the workgroup's four waves in turn; the waves' sums are added in wave order, so part holds gridDim.x partial sums per pair:
// part[(p * gridDim.x + block) * 256 + i * 16 + j].  No atomics: the same inputs give the same bits.
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256, 2) void k_solve_quad_cross(const SolveSeg* __restrict__ segs, const long* __restrict__ seg_off, int nseg,
                                                             const double* __restrict__ arch, long panel, QuadGroup G,
                                                             double* __restrict__ part) {
    __shared__ double red[4 * 256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, kk = lane >> 4;
    const bool on0 = G.blk[0] >= 0, on1 = G.blk[1] >= 0, on2 = G.blk[2] >= 0, on3 = G.blk[3] >= 0;
    const double* p0 = arch + (long)(on0 ? G.blk[0] : 0) * panel + lane;
    const double* p1 = arch + (long)(on1 ? G.blk[1] : 0) * panel + lane;
    const double* p2 = arch + (long)(on2 ? G.blk[2] : 0) * panel + lane;
    const double* p3 = arch + (long)(on3 ? G.blk[3] : 0) * panel + lane;
    d4 a01 = {0, 0, 0, 0}, a02 = a01, a03 = a01, a12 = a01, a13 = a01, a23 = a01;
    // one chunk: the four panels' loads first, then the six products
#define MRA_QUAD_CROSS_CHUNK(K0)                                                                                                     \
    {                                                                                                                                \
        const bool in = (K0) + kk < n;                                                                                               \
        const long e = off + (long)(K0) * 16;                                                                                        \
        const double v0 = (in && on0) ? gld(p0 + e) : 0.0;                                                                           \
        const double v1 = (in && on1) ? gld(p1 + e) : 0.0;                                                                           \
        const double v2 = (in && on2) ? gld(p2 + e) : 0.0;                                                                           \
        const double v3 = (in && on3) ? gld(p3 + e) : 0.0;                                                                           \
        const double s0 = sg * v0, s1 = sg * v1, s2 = sg * v2;                                                                       \
        a01 = mfma16(s0, v1, a01); a02 = mfma16(s0, v2, a02); a03 = mfma16(s0, v3, a03);                                             \
        a12 = mfma16(s1, v2, a12); a13 = mfma16(s1, v3, a13); a23 = mfma16(s2, v3, a23);                                             \
    }
    // A leaf's segment is a few chunks per wave, so a wave meets a new descriptor every few loads: the next segment's is read while
    // this one's rows are on their way (measured neutral at c3 and c5, DESIGN.md section 20: the wait is for the rows).
    int sgi = blockIdx.x;
    int n = 0, sign = 1;
    long off = 0;
    if (sgi < nseg) { n = segs[sgi].n; sign = segs[sgi].sign; off = seg_off[sgi] * 16; }
    while (sgi < nseg) {
        const int nxt = sgi + gridDim.x;
        int n_nxt = 0, sign_nxt = 1;
        long off_nxt = 0;
        if (nxt < nseg) { n_nxt = segs[nxt].n; sign_nxt = segs[nxt].sign; off_nxt = seg_off[nxt] * 16; }
        const double sg = (double)sign;
#pragma unroll 2
        for (int k0 = 4 * w; k0 < n; k0 += 16) MRA_QUAD_CROSS_CHUNK(k0)
        sgi = nxt; n = n_nxt; sign = sign_nxt; off = off_nxt;
    }
#undef MRA_QUAD_CROSS_CHUNK
    const int i = lane & 15;
#define MRA_QUAD_CROSS_FOLD(P, ACC)                                                                                                  \
    if (G.out[P]) {                                                                                                                  \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) red[w * 256 + (kk + 4 * j) * 16 + i] = ACC[j];                                 \
        __syncthreads();                                                                                                             \
        part[((long)(P) * gridDim.x + blockIdx.x) * 256 + threadIdx.x] =                                                             \
            ((red[threadIdx.x] + red[256 + threadIdx.x]) + red[512 + threadIdx.x]) + red[768 + threadIdx.x];                         \
        __syncthreads();                                                                                                             \
    }
    MRA_QUAD_CROSS_FOLD(0, a01) MRA_QUAD_CROSS_FOLD(1, a02) MRA_QUAD_CROSS_FOLD(2, a03)
    MRA_QUAD_CROSS_FOLD(3, a12) MRA_QUAD_CROSS_FOLD(4, a13) MRA_QUAD_CROSS_FOLD(5, a23)
#undef MRA_QUAD_CROSS_FOLD
}
#endif
// The partial sums of a group's pairs folded in block order, one workgroup per pair; the tile of pair (a, b) and its mirror go into the
// dense ldq x ldq matrix Q (tiles on the diagonal are not touched: k_solve_quad_part / k_solve_quad_sum own them).
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256) void k_solve_quad_cross_sum(const double* __restrict__ part, int nblk, QuadGroup G, double* __restrict__ Q,
                                                              int ldq) {
    int a = -1, b = -1, want = 0;
    if (blockIdx.x == 0) { a = G.blk[0]; b = G.blk[1]; want = G.out[0]; }
    if (blockIdx.x == 1) { a = G.blk[0]; b = G.blk[2]; want = G.out[1]; }
    if (blockIdx.x == 2) { a = G.blk[0]; b = G.blk[3]; want = G.out[2]; }
    if (blockIdx.x == 3) { a = G.blk[1]; b = G.blk[2]; want = G.out[3]; }
    if (blockIdx.x == 4) { a = G.blk[1]; b = G.blk[3]; want = G.out[4]; }
    if (blockIdx.x == 5) { a = G.blk[2]; b = G.blk[3]; want = G.out[5]; }
    if (!want) return;
    double acc = 0.0;
    for (int k = 0; k < nblk; ++k) acc += part[((long)blockIdx.x * nblk + k) * 256 + threadIdx.x];
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
    Q[(long)(a * 16 + i) * ldq + b * 16 + j] = acc;
    Q[(long)(b * 16 + j) * ldq + a * 16 + i] = acc;
}
#endif

// ---- trend (mra_trend_fit): universal-kriging mean and variance by padded row ------------------------------
// m: (1 + p) x P kriging means of [y | X] (row 0: m_y), X: p x P design matrix, both by padded row.  h = x(s) - m_X(s);
// mean = m_y + h^T beta, var = var_pass + |L^-1 h|^2 with A = L L^T = X^T K^-1 X.  One row per lane, one wave per workgroup: L^-1
// (64 x 64 doubles, row stride 64) and the lanes' h (hs[j * 64 + lane]: no bank conflicts) in LDS.  Unreported rows get exactly 0.
#define MRA_TREND_LD 64
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(64) void k_trend_rows(const double* __restrict__ m, const double* __restrict__ X, const double* __restrict__ beta,
                                                   const double* __restrict__ Linv, const double* __restrict__ var_pass,
                                                   const unsigned char* __restrict__ rep, int p, long P, double* __restrict__ mean,
                                                   double* __restrict__ var) {
    __shared__ double Ls[MRA_TREND_LD * MRA_TREND_LD];
    __shared__ double hs[(MRA_TREND_LD - 1) * 64];
    const int lane = threadIdx.x;
    for (int e = lane; e < p * MRA_TREND_LD; e += 64) Ls[e] = Linv[e];
    const long s = (long)blockIdx.x * 64 + lane;
    const bool in = s < P;
    double mu = in ? m[s] : 0.0;
    for (int j = 0; j < p; ++j) {
        const double h = in ? X[(long)j * P + s] - m[(long)(j + 1) * P + s] : 0.0;
        hs[j * 64 + lane] = h;
        mu = __builtin_fma(h, beta[j], mu);
    }
    __syncthreads();
    double add = 0.0;
    for (int i = 0; i < p; ++i) {
        double wi = 0.0;
        for (int j = 0; j <= i; ++j) wi = __builtin_fma(Ls[i * MRA_TREND_LD + j], hs[j * 64 + lane], wi);
        add = __builtin_fma(wi, wi, add);
    }
    if (!in) return;
    const bool r = rep[s] != 0;
    mean[s] = r ? mu : 0.0;
    var[s] = r ? var_pass[s] + add : 0.0;
}
#endif

// ---- rows: mean[tile, 0:16] = W[tile, anc] beta + C(tile, obs) q, one wave per 16-row tile ---------------------------------------
// The covariance is evaluated on the fly as the A operand (lane (r, q) evaluates C(x_row r, x_obs q + 4 s)); the Kanter taper goes
// through sinpi / cospi (no range-reduction table on the stack).  out: 16 x P, column-major blocks (column c at out + c P);
// unreported rows are written as 0.
template <int MODE>
__device__ __forceinline__ double solve_cov(const KernelParams& kp, double D2) {
    if (MODE == 3) {
        const double D = fmin(sqrt_pos(D2) * kp.c_inv_l, 2.0);
        const double p2 = 6.283185307179586 * D;
        const double v = (1.0 - D) * sinpi(2.0 * D) / p2 + 0.3183098861837907 * (1.0 - cospi(2.0 * D)) / p2;
        return kp.amp * ((D == 0.0) ? 1.0 : ((D > 1.0) ? 0.0 : v));
    }
    return cov_of_dist2<MODE>(kp, D2);
}

// ... of a pair of locations: the same expression as before for the modes that are functions of the distance, cov_local for mode 6
template <int DIM, int MODE>
__device__ __forceinline__ double solve_cov_pair(const KernelParams& kp, const double* __restrict__ xa, const double* __restrict__ xb) {
    if constexpr (MODE == 6) return cov_local<DIM>(kp, xa, xb);
    else return solve_cov<MODE>(kp, pair_dist2<DIM>(xa, xb, kp.circular));
}

template <int DIM, int MODE>
__global__ __launch_bounds__(256, 4) void k_solve_rows(const SolveLeaf* __restrict__ lv, const int* __restrict__ tile_leaf,
                                                       const double* __restrict__ W, long ldw, const double* __restrict__ X,
                                                       const unsigned char* __restrict__ rep, KernelParams kp,
                                                       double* __restrict__ out, long P) {
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile * 16 >= P) return;
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const long row0 = tile * 16;
    d4 acc = {0, 0, 0, 0};
    const int t = tile_leaf[tile];
    if (t >= 0) {
        const SolveLeaf L = lv[t];
        for (int k0 = 0; k0 < L.anc; k0 += 16) {
            const d4 a = load_rowlane(W + row0 * ldw + L.a0 + k0, ldw, r, q);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma16(a[s], gld(L.gb + (long)(k0 + q + 4 * s) * 16 + r), acc);
        }
        double xr[DIM];
#pragma unroll
        for (int e = 0; e < DIM; ++e) xr[e] = gld(X + (row0 + r) * DIM + e);
        for (int o0 = 0; o0 < L.nop; o0 += 16) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = o0 + q + 4 * s;
                const int o = gldi(L.obs + k);
                double xo[DIM];
#pragma unroll
                for (int e = 0; e < DIM; ++e) xo[e] = gld(X + (long)(o >= 0 ? o : 0) * DIM + e);
                const double cv = solve_cov_pair<DIM, MODE>(kp, xr, xo);
                acc = mfma16(o >= 0 ? cv : 0.0, gld(L.uy + (long)k * 16 + r), acc);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long row = row0 + q + 4 * j;
        gst(out + (long)r * P + row, rep[row] ? acc[j] : 0.0);
    }
}

// ---- glue ------------------------------------------------------------------------------------------------------------------------
// pseudo-data of a block of conditional draws, 16 columns at once: Yb[s][p] = y[p] - x_s[p] - sqrt(R) eps_s[p] at observed rows, 0
// elsewhere (the solve reads observed rows only)
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256) void k_solve_pseudo(const double* __restrict__ y, const double* __restrict__ x, SampleZ zs, long slot0,
                                                      double sqrtR, double* __restrict__ Yb, long P) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const double yp = y[p];
    const bool ob = yp == yp && fabs(yp) != __builtin_inf();
    for (int s = 0; s < 16; ++s)
        Yb[(long)s * P + p] = (ob && s < zs.ns) ? yp - x[(long)s * P + p] - sqrtR * sample_z(zs, slot0 + p, s) : 0.0;
}
#endif
// the same with a noise vector: sd[p] = sqrt(r_p) by padded row
#ifndef MRA_COV_TEMPLATES_ONLY      /* non-template kernels: defined once, in the translation unit of mra_launch_solve.hip */
__global__ __launch_bounds__(256) void k_solve_pseudo_rows(const double* __restrict__ y, const double* __restrict__ x, SampleZ zs, long slot0,
                                                           const double* __restrict__ sd, double* __restrict__ Yb, long P) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const double yp = y[p];
    const bool ob = yp == yp && fabs(yp) != __builtin_inf();
    const double sdp = sd[p];
    for (int s = 0; s < 16; ++s)
        Yb[(long)s * P + p] = (ob && s < zs.ns) ? yp - x[(long)s * P + p] - sdp * sample_z(zs, slot0 + p, s) : 0.0;
}
__global__ __launch_bounds__(256) void k_solve_addmean(double* __restrict__ x, const double* __restrict__ mean, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] += mean[i];
}
#endif
