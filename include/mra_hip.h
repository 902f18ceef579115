/*
 * mra_hip.h - C ABI of libmra_hip.so: the MI355X (gfx950) implementation of pyMRA's per-node
 * prior/posterior inference hot path.
 *
 * The reference (marcinjurek/pyMRA) is pure Python and has no FFI boundary of its own: all of the
 * work below happens inside its MRATree constructor.  Each entry point states which reference
 * interface (file:line under the reference checkout) it stands in for.  The Python facade that a
 * pyMRA user sees (pymra_amd.MRATree) binds these with ctypes; INTEGRATION.md shows the stub a
 * pyMRA maintainer would add.
 *
 * Conventions: every function returns 0 on success and a negative MRA_ERR_* code on failure and
 * never throws (a C++ exception from inside the library, std::bad_alloc included, comes back as
 * MRA_ERR_INVALID with its what() text); mra_last_error() gives the message.  Host pointers
 * passed in are copied before the call returns and never retained.  Results are written only
 * into caller-allocated host buffers.
 * A plan is bound to one GPU and one internal HIP stream; it is not thread-safe.
 * All floating point data is IEEE binary64, all row indices refer to the caller's padded,
 * leaf-ordered row space (see mra_topology).
 */
#ifndef MRA_HIP_H
#define MRA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRA_OK                 0
#define MRA_ERR_INVALID       -1   /* bad argument / inconsistent topology                      */
#define MRA_ERR_HIP           -2   /* a HIP runtime call failed (no GPU, out of memory, ...)    */
#define MRA_ERR_NOT_SPD       -3   /* a Cholesky pivot was <= 0 or NaN (reference: pdb prompt,   */
                                   /*   pyMRA/MRANode.py:386-390)                               */
#define MRA_ERR_STATE         -4   /* call order violated (e.g. run before set_obs)             */
#define MRA_ERR_COMM          -5   /* RCCL failure                                              */

/* stationary kernels evaluated on the device (pyMRA/MRATools.py:256-301) */
#define MRA_KERNEL_EXP         0   /* ExpCovFun      exp(-D/l)                          :265-269 */
#define MRA_KERNEL_MATERN32    1   /* Matern32       sig (1+sqrt3 D/l) exp(-sqrt3 D/l)  :289-293 */
#define MRA_KERNEL_MATERN52    2   /* Matern52                                          :281-285 */
#define MRA_KERNEL_GAUSSIAN    3   /* GaussianCovFun sig exp(-D^2/(2 l^2))              :297-301 */
#define MRA_KERNEL_IDEN        4   /* Iden           [D == 0]                           :256-262 */
#define MRA_KERNEL_KANTER      5   /* KanterCovFun   compact taper, radius = l          :305-324 */
#define MRA_KERNEL_MATERN      6   /* Matern(nu)     sig 2^(1-nu)/Gamma(nu) t^nu K_nu(t), t = sqrt(2 nu) D/l :273-277 */
#define MRA_KERNEL_SUM         7   /* sum of 1..MRA_SUM_MAX of EXP, MATERN32, MATERN52, GAUSSIAN, IDEN: a nested model */
#define MRA_SUM_MAX            4
#define MRA_KERNEL_LOCAL       8   /* local ranges (nonstationary): the last coordinate column is a range lam(s) > 0;
                                      sig (la lb / q)^(ds/2) k0(D / (l sqrt q)), q = (la^2 + lb^2) / 2, k0 = EXP, MATERN32, MATERN52 or GAUSSIAN */
#define MRA_KERNEL_HOST        100 /* values supplied block by block (any cov callable or a dense
                                      matrix, pyMRA/MRANode.py:73-80, 381-384)                   */

/* mra_run flags */
#define MRA_RUN_LIKELIHOOD     1u  /* d and u                 (MRATree.getLikelihood, MRATree.py:82-84) */
#define MRA_RUN_PREDICT        2u  /* + predictive mean / var (MRATree.predict,       MRATree.py:90-94) */

typedef struct mra_plan mra_plan;

/*
 * The tree that pyMRA's Node.__init__ recursion (pyMRA/MRANode.py:23-115) would build, flattened.
 * Rows are in depth-first leaf order and every leaf's row range is padded to a multiple of 16
 * (phantom rows); node i owns rows [node_row0[i], node_row1[i]); nodes are numbered level by
 * level: level m owns nodes level_ptr[m] .. level_ptr[m+1]-1; node 0 is the root.
 * knot_rows[knot_ptr[i] .. knot_ptr[i+1]) are the padded-row positions of node i's knots
 * (pyMRA/MRANode.py:36-45, 179-205); for a leaf they are informational only.
 * cw[m] = knot-block width of the non-leaf nodes of level m, a multiple of 16 (0: none).
 */
typedef struct {
    int64_t        P;            /* padded rows                                    */
    int32_t        d;            /* dimension of the coordinates the covariance is evaluated on: 1, 2 or 3 (3: chordal distance on a
                                  * sphere, or 3-D Euclidean).  The tree arrays below do not depend on it: the partition may
                                  * have been built on other coordinates (lon/lat for points on a sphere)            */
    int32_t        n_levels;
    int32_t        n_nodes;
    const int64_t *level_ptr;    /* [n_levels + 1]                                 */
    const int64_t *node_row0;    /* [n_nodes]                                      */
    const int64_t *node_row1;    /* [n_nodes]                                      */
    const uint8_t *node_leaf;    /* [n_nodes]                                      */
    const int32_t *node_parent;  /* [n_nodes], -1 for the root                     */
    const int32_t *child_ptr;    /* [n_nodes + 1]                                  */
    const int32_t *child_list;   /* [child_ptr[n_nodes]]                           */
    const int64_t *knot_ptr;     /* [n_nodes + 1]                                  */
    const int64_t *knot_rows;    /* [knot_ptr[n_nodes]]                            */
    const int32_t *cw;           /* [n_levels]                                     */
} mra_topology;

/* Number of usable GPUs (0 if none); never fails. */
int mra_device_count(void);

/* Replaces: the allocation side of MRATree.__init__ -> Node(...) (pyMRA/MRATree.py:69).
 * device: HIP device ordinal.  The topology arrays are copied. */
int mra_plan_create(mra_plan **plan, const mra_topology *topo, int device);
int mra_plan_destroy(mra_plan *plan);

/* Replaces: the `locs` argument of MRATree (pyMRA/MRATree.py:23-28).
 * locs_perm: P x d row-major, padded leaf order (phantom rows must hold a valid location). */
int mra_plan_set_locs(mra_plan *plan, const double *locs_perm);

/* Anisotropic and space-time covariances (no counterpart in the reference, whose kernels take dist(locs, locs2), pyMRA/MRATools.py:229-253;
 * DESIGN.md section 19): every device kernel evaluates value = scale * k(h; l, sig) with h = |A (a - b)|.  Geometric anisotropy (a ratio
 * and an angle), per-axis ranges and (x, y, t) data with a temporal range of its own are all this.
 * h = |A (a - b)|: A is d x d row-major (d = the topology's d), NULL = no metric (the identity).
 * The metric is applied in front of the kernels, once per call: the plan keeps the caller's coordinates x in one more P x d array (allocated
 * by the first non-NULL call, released by NULL) and hands every kernel t = A x, row i computed as
 *     acc = A[i][0] * x[0];  for k = 1 .. d-1: acc = fma(A[i][k], x[k], acc)
 * by one function on the device and on the host (the knot coordinates of regular trees, the sites of the site calls): the same bits
 * everywhere, and x itself for A = I.  No kernel of a pass changes, and a plan that never sets a metric allocates and launches nothing new.
 * The metric is a property of the plan, as the kernel is: it survives mra_plan_set_locs* (which then take the caller's coordinates and
 * transform them again) and mra_plan_set_obs*.  mra_predict_sites, mra_sites_cov and mra_sample_sites take their sites in the caller's
 * coordinates and transform them the same way (a site that is a tree location still reproduces that row bit for bit; the duplicate
 * collapse of mra_sample_sites compares the transformed coordinates).  NULL puts the caller's coordinates back bit for bit.
 * As after mra_plan_set_kernel the retained factors, the kept prior and the kept residual are dropped; y, the mask, the noise vector, the
 * leaf lists and every option stay.  Allowed on sharded plans: every rank sets the same A (the rows are the rank's own).
 * MRA_ERR_STATE before mra_plan_set_locs.  MRA_ERR_INVALID, checked on the host before anything changes: an entry of A that is not
 * finite; a determinant that is 0 or not finite; a non-NULL A while the kernel is circular (and mra_plan_set_kernel with circular != 0
 * while a metric is set: the torus has period 1 in the raw coordinate); a non-NULL A on an MRA_KERNEL_HOST plan (and selecting
 * MRA_KERNEL_HOST while a metric is set: those plans never read coordinates).  mra_get_buffer(13) returns the coordinates the kernels read. */
int mra_plan_set_metric(mra_plan *plan, const double *A);

/* Replaces: the `obs` and `R` arguments of MRATree (pyMRA/MRATree.py:23, 61-62; NaN = missing,
 * pyMRA/MRANode.py:415).  y_perm: P values, padded leaf order, NaN for missing and for phantom rows.
 * R: scalar nugget variance (the reference requires a Python float, pyMRA/MRANode.py:85-88). */
int mra_plan_set_obs(mra_plan *plan, const double *y_perm, double R);

/* Replaces: the non-float `R` of the reference, a matrix that Node.__init__ slices per child (pyMRA/MRANode.py:85-88) and that its
 * leaves then cannot use (R*np.eye, (1/R)*H.T*H, :415-430) - here its diagonal: per-observation noise variances,
 * y_p = x(s_p) + eps_p, eps_p ~ N(0, r_p).  Every leaf factorises C = v_M(o,o) + diag(r_o); the likelihood, the predictions, mra_solve,
 * mra_cov_apply, mra_predict_sites, mra_sites_cov, mra_sample_sites and sharded passes are what they are with that C, and conditional
 * draws of mra_sample use sqrt(r_p) eps_p as the noise of row p (same noise slots).  With r_p = R at every observed row every result is
 * bit for bit the scalar one: the leaves' C is written as v + 0 and the diagonal then takes r in one rounding, as v + R does.
 * r_perm: P values, padded leaf order, read only at the rows the plan observes (finite y); values elsewhere, NaN included, are ignored.
 * NULL returns to the scalar R of the last mra_plan_set_obs.  Call it after mra_plan_set_obs (MRA_ERR_STATE before); a later
 * mra_plan_set_obs* drops the vector (its scalar holds again: the mask may have changed).  MRA_ERR_INVALID for a value that is negative
 * or not finite at an observed row, checked on the host before anything changes.  y, the mask, the leaf lists and every option stay;
 * the retained factors do not (as after any set_*, the next call on them factorises once).  Allowed on sharded plans (the rows are the
 * rank's own) and on MRA_KERNEL_HOST plans.  A pass with a vector set launches one more kernel (k_leaf_noise); a pass without one is
 * unchanged.  mra_plan_set_noise_rows: r in the CALLER's row order (N values), gathered through the topology's src[P] as
 * mra_plan_set_locs_rows gathers the locations. */
int mra_plan_set_noise(mra_plan *plan, const double *r_perm);
int mra_plan_set_noise_rows(mra_plan *plan, const double *r, const int64_t *src);

/* Non-Gaussian data by a Laplace approximation (no counterpart in the reference, whose observations are Gaussian): the posterior
 * mode of x given z_p ~ p(. | eta_p), eta_p = x(s_p) + offset_p at the rows the plan observes, found by Newton / IRLS on the device.
 *   MRA_FAMILY_GAUSSIAN  N(eta, aux):              g = (z - eta) / aux,  D = 1 / aux,        start x0 = z - offset
 *   MRA_FAMILY_POISSON   Poisson(e^eta):           g = z - e^eta,        D = e^eta,          start x0 = log(z + 1/2) - offset
 *   MRA_FAMILY_BINOMIAL  Bin(aux, logistic(eta)):  g = z - aux p,        D = aux p (1 - p),  start x0 = log((z + 1/2) / (aux - z + 1/2)) - offset
 * (g = d log p / d eta, D = -d2 log p / d eta2, floored at 2^-40).  One iteration from x: t_p = x_p + g_p / D_p and r_p = 1 / D_p go
 * into the plan's y and noise at the observed rows (one launch), one likelihood + predict pass gives x^ = its mean there, and
 * step = max |x^ - x| (two launches, a fixed number of partial results in a fixed order: the same inputs give the same bits).  The
 * call stops after the pass with step <= tol * max(1, max |x^|), or after max_iter passes (MRA_OK, info[7] = 0).  Plain Newton: no
 * damping, no step control.  The Gaussian family's t = z - offset and r = aux do not depend on x: its second pass repeats the first.
 * z_perm, aux_perm, offset_perm, x0_perm: P values each, padded leaf order.  z must be finite exactly where the plan observes (the mask
 * is that of the last mra_plan_set_obs: the call builds no leaf lists and keeps every option; rows outside every leaf are nobody's and
 * are not read).  aux_perm may be NULL for Poisson; offset_perm NULL: 0; x0_perm NULL: the start of the table.
 * info[8]: [0] d = log|Sigma + D^-1| and [1] u = t^T (Sigma + D^-1)^-1 t of the last pass; [2] -2 sum log p(z_p | eta^_p), every
 * normalising constant included; [3] sum log D_p; [4] sum D_p (t_p - x^_p)^2 ([3], [4]: D and t of the last pass); [5] passes run;
 * [6] the last step; [7] converged, 1 or 0.  -2 log q(z) of the Laplace approximation is [0] + [1] + [2] + [3] - [4].
 * MRA_ERR_STATE without set_locs, set_obs and set_kernel.  MRA_ERR_INVALID, checked on the host in this order before anything
 * changes: an unknown family; a mask that differs from the plan's; at an observed row z < 0 (the two count families), (binomial) aux < z or aux <= 0,
 * (Gaussian) aux <= 0, a non-finite aux, offset or x0 where one is read; max_iter < 1; tol not > 0; NULL z or info; a sharded plan.
 * A pass's MRA_ERR_NOT_SPD propagates, with that pass's r in the plan.  An iterate that leaves the doubles (e^eta = inf: t = NaN,
 * r = 0; undamped Newton from a poor start on counts in the thousands gets there) never comes back as converged: a pass reads a NaN y
 * as 0, and r = 0 at a row that is a knot of a node above the leaves has no positive pivot, so such a pass is as a rule refused
 * MRA_ERR_NOT_SPD - the same holds for any r below the rounding of that pivot, about 1e-16 of the prior variance (a Poisson mean
 * near 1e16) - and a pass that does come back with a step that is NaN or inf ends the call: MRA_OK, info[5] = the passes including
 * it, info[6] = that step, info[7] = 0.  Afterwards the plan is a plan after mra_plan_set_obs(t) + mra_plan_set_noise(r) +
 * mra_run(LIKELIHOOD | PREDICT): mra_get_likelihood / mra_get_predict give the last pass, mra_get_buffer(10) gives r, and the calls on
 * the retained factors serve the Laplace posterior N(x^, (Sigma^-1 + D)^-1) (they factorise once first).  The next mra_plan_set_obs
 * returns the plan to the Gaussian model.  Works on MRA_KERNEL_HOST plans. */
#define MRA_FAMILY_GAUSSIAN 0
#define MRA_FAMILY_POISSON  1
#define MRA_FAMILY_BINOMIAL 2
int mra_plan_fit_laplace(mra_plan *plan, int family, const double *z_perm, const double *aux_perm, const double *offset_perm,
                         const double *x0_perm, int max_iter, double tol, double *info);

/* Replaces: the `cov` callable when it is one of pyMRA's stationary kernels
 * (pyMRA/MRATools.py:256-301).  params = {l, sig, scale[, circular]}; value = scale * k(D; l, sig);
 * circular != 0 (1-D only): D = min(|a-b|, 1-|a-b|), the torus branch of dist() (MRATools.py:232-239).
 * kind == MRA_KERNEL_MATERN: params = {l, sig, scale, circular, nu}, n_params >= 5, 0.1 <= nu <= 5 (sklearn's parametrisation,
 * nu = 1.5 and 2.5 are Matern32 and Matern52).  The plan builds a table of 191 quadrature nodes for nu on the host and keeps it in a
 * device buffer of its own, rebuilt only when nu changes.  Such plans take the level-by-level prior (mra_get_route) and every call on the
 * retained factors.  Every refusal of this call comes before anything of the plan changes (the previous kernel and everything retained
 * stand): circular distances on a plan that is not 1-D or has a metric, l <= 0, and MRA_ERR_INVALID for an
 * unknown kind, n_params < 3 and, for MRA_KERNEL_MATERN, n_params < 5, l <= 0 and a nu that is not finite or outside [0.1, 5].
 * kind == MRA_KERNEL_SUM: value = scale * sum over c < K of sig_c k_c(D; l_c), a nested model of 1 <= K <= MRA_SUM_MAX structures that share
 * the plan's distance (dimension, metric, circular).  params = {K, 0, scale, circular, kind_0, l_0, sig_0, ..., kind_{K-1}, l_{K-1},
 * sig_{K-1}}, n_params >= 4 + 3 K; kind_c is MRA_KERNEL_EXP, MATERN32, MATERN52, GAUSSIAN or IDEN, each evaluated by the formula of its own
 * kind with sig_c as its sill (for EXP and IDEN too: sig_c = 1 is the single kind) - an IDEN component is sig_c at D == 0 and exactly 0
 * elsewhere, a micro-scale part of the field, not noise.  The plan derives one record of 6 doubles per component {submode, c / l,
 * 1 / (2 l^2), a1, a2, scale sig_c} into a device buffer of its own (mra_get_buffer 17), uploaded on every such call - a few hundred
 * bytes, all that an optimiser's step over ranges and sills sends.  Such plans take the level-by-level prior (mra_get_route) and every
 * call on the retained factors.  MRA_ERR_INVALID, before anything of the plan changes: K not an integer in 1..MRA_SUM_MAX, n_params <
 * 4 + 3 K, a component kind outside the five (MRA_KERNEL_KANTER and MRA_KERNEL_MATERN are no components), l_c <= 0 or not finite,
 * sig_c < 0 or not finite, circular on a plan that is not 1-D or has a metric.
 * kind == MRA_KERNEL_LOCAL: a nonstationary covariance after Paciorek & Schervish (2006) with isotropic local kernels.  The plan's
 * coordinates have d = 2 columns (x, lam) or d = 3 columns (x, y, lam): ds = d - 1 spatial coordinates, on which the distance D is
 * taken, and the local range lam(s) > 0 of the location in the LAST column (the same holds for the sites of mra_predict_sites,
 * mra_sites_cov and mra_sample_sites).  With q = (la^2 + lb^2) / 2,
 *     value = scale * sig * (la lb / q)^(ds / 2) * k0(D / (l sqrt(q))),     k0 the base kind at range 1,
 * params = {l, sig, scale, 0, base_kind}, n_params >= 5, base_kind MRA_KERNEL_EXP, MATERN32, MATERN52 or GAUSSIAN (each a scale mixture
 * of Gaussians, which the validity theorem needs); sig is the sill for every base.  l multiplies the whole range field, so an
 * optimiser's step over (l, sig) sends these parameters and nothing else; a constant field lam = lam0 is the stationary kernel of
 * range l lam0; value(a, a) = scale sig exactly.  Such plans take the level-by-level prior (mra_get_route) and every call on the
 * retained factors.  MRA_ERR_INVALID, before anything of the plan changes: a plan with d = 1, a base kind outside the four,
 * circular != 0, l <= 0 or not finite, sig < 0 or not finite, a plan with a metric (mra_plan_set_metric with a non-NULL A on such a
 * plan is refused as well: A would mix the range into the distance), and a last column that is not positive and finite at every
 * padded row - checked on the host by whichever of mra_plan_set_locs[_rows] and this call comes second (the plan remembers the
 * smallest value of that column, nothing else).
 * kind == MRA_KERNEL_HOST (params ignored, call after mra_plan_set_obs): covariance values come from
 * mra_plan_set_cov_block. */
int mra_plan_set_kernel(mra_plan *plan, int kind, const double *params, int n_params);

/* Diagnostics: out[i] = scale * k_kind(D[i]; l, sig) evaluated by the device code that the inference
 * kernels inline - the device counterpart of ExpCovFun/Matern32/... applied to D = dist(locs, locs2)
 * (pyMRA/MRATools.py:229-301).  MRA_KERNEL_MATERN takes params = {l, sig, scale, circular, nu} and
 * MRA_KERNEL_SUM {K, 0, scale, circular, kind_0, l_0, sig_0, ...} as mra_plan_set_kernel does. */
int mra_eval_kernel(int kind, const double *params, int n_params, const double *D, int64_t n, double *out);

/* Diagnostics, MRA_KERNEL_LOCAL: out[i] = the value for a pair at distance D[i] (over ds = 1 or 2 spatial dimensions) with the local
 * ranges la[i] and lb[i], evaluated by the device function that the inference kernels inline.  params = {l, sig, scale, 0,
 * base_kind} as mra_plan_set_kernel takes them; D, la, lb and out are arrays of n.  A range of 1e150 or more - a phantom knot's -
 * gives exactly 0.  (mra_eval_kernel refuses this kind: it is no function of the distance alone.) */
int mra_eval_kernel_local(const double *params, int n_params, int ds, const double *D, const double *la, const double *lb, int64_t n,
                          double *out);

/* Replaces: the `cov` callable for anything else (MRA_KERNEL_HOST): the host evaluates
 * C(S_j, Q_j) for a non-leaf node (N_j x rank, row-major, pyMRA/MRANode.py:384) or
 * C(S_j, O_j) for a leaf (N_j x n_obs_j; O_j = the leaf's observed rows in ascending row order)
 * and hands it over.  diag: C(x,x) for each of the node's N_j rows (leaves only, else NULL). */
int mra_plan_set_cov_block(mra_plan *plan, int32_t node, const double *C, int64_t n_rows,
                           int64_t n_cols, const double *diag);

/* Replaces: everything Node.__init__ computes - calculatePrior (pyMRA/MRANode.py:378-395) for
 * every node top-down, calculatePosterior (:403-523) bottom-up.  Blocking. */
int mra_run(mra_plan *plan, uint32_t flags);

/* Replaces: MRATree.getLikelihood (pyMRA/MRATree.py:82-84): lik = *d + *u
 * (root.d, root.u of pyMRA/MRANode.py:456-468). */
int mra_get_likelihood(mra_plan *plan, double *d, double *u);

/* Replaces: MRATree.predict (pyMRA/MRATree.py:90-94): root.mean and root.var
 * (pyMRA/MRANode.py:510-520) in padded leaf order, P values each. */
int mra_get_predict(mra_plan *plan, double *mean_perm, double *var_perm);

/* Simulation from the model (the reference's dense-Cholesky simulate1D / simulateGRF, pyMRA/MRATools.py:395-484, at any size):
 * exact draws from the MRA prior covariance Sigma = sum_j B_j k_j B_j^T of the reported rows, or, with MRA_SAMPLE_CONDITIONAL,
 * from the posterior given the plan's observations and noise r ("conditioning by kriging": x + mean_MRA(y - x_o - sqrt(r_o) eps), r_o = R or the vector of mra_plan_set_noise,
 * one likelihood + predict pass per conditional draw).  A prior draw is
 *     x = sum_{non-leaf j} W^m(j)[rows_j] z_j + sum_{leaf j} L_j zeta_j,   L_j L_j^T = v_M(K_j, K_j)  (K_j: the leaf's knot rows)
 * Latent slots (mra_sample_slots gives their number, Kn + 2 P):
 *     [0, Kn)            the non-leaf nodes in node order, cw[level] slots each, in knot-column order (phantom knots: unused)
 *     [Kn, Kn + P)       leaf terms by padded row; read only at the knot rows of the row's leaf
 *     [Kn + P, Kn + 2P)  observation noise by padded row; read only with MRA_SAMPLE_CONDITIONAL, at observed rows
 * z: NULL = draw on the device: slot k of sample s is Philox4x32-10 with key = seed (lo, hi) and counter = (k lo, k hi, s' lo, s' hi),
 * s' = sample0 + s, output words w0..w3; a = w0 + 2^32 w1, b = w2 + 2^32 w3, u1 = ((a >> 11) + 0.5) 2^-53, u2 likewise from b,
 * z = sqrt(-2 log u1) cospi(2 u2) - a pure function of (seed, slot, sample).  Otherwise z is n_samples x n_slots, row-major.
 * out: n_samples x P, padded leaf order; unreported rows (phantoms, rows a 1-D split drops) are exactly 0.
 * Needs set_locs, set_obs and set_kernel (MRA_ERR_STATE); MRA_ERR_INVALID for MRA_KERNEL_HOST plans, sharded plans,
 * n_samples < 0, sample0 < 0 and sample0 + n_samples - 1 > 2^63 - 1 (sample numbers are non-negative int64);
 * MRA_ERR_NOT_SPD when a leaf's v_M(K, K) does not factor (no jitter is added).  The device y and every option
 * are as the caller left them afterwards, mra_get_likelihood / mra_get_predict still return the last mra_run's values
 * (mra_get_timers / mra_get_kernel_stats describe the sampler's own passes).  Blocking. */
#define MRA_SAMPLE_CONDITIONAL 1u
int mra_sample_slots(mra_plan *plan, int64_t *n_slots);
int mra_sample(mra_plan *plan, uint32_t flags, int64_t n_samples, uint64_t seed, int64_t sample0,
               const double *z, double *out);

/* Factor once, solve many (no counterpart in the reference, which re-runs calculatePosterior for every observation vector,
 * pyMRA/MRANode.py:403-523): the leaves' L_c and Ut and the fronts' Lt and Zt of one likelihood pass are a complete factorisation of
 * the posterior precision of the MRA weights; they do not depend on y.  For n_cols observation vectors Y (n_cols x P, row-major:
 * vector k at Y + k P, padded leaf order, read at the plan's OBSERVED rows only - the mask of the last set_obs)
 *     mean (n_cols x P, or NULL): mean[k] = E[x | Y[k] at the observed rows] = the mean mra_run + mra_get_predict give for y = Y[k];
 *                                 unreported rows (phantoms, rows a 1-D split drops) are exactly 0
 *     quad (n_cols x n_cols, or NULL): Y_o^T (Sigma_MRA[o, o] + D)^-1 Y_o, D = R I or diag(r_o) of mra_plan_set_noise, so that quad[k][k] is the u of mra_get_likelihood for
 *                                 y = Y[k] (the log-determinant d does not depend on y)
 * Columns are processed in blocks of 16 (the N of v_mfma_f64_16x16x4_f64).  quad is returned BLOCK-DIAGONAL: entries whose row and
 * column lie in the same block of 16 columns (k / 16 equal) are computed, all others are set to NaN - a cross-block entry needs the
 * forward sweeps of both blocks at once.  Callers that need a full quad of more than 16 columns pass MRA_SOLVE_FULL_QUAD (below).
 * The first call (and the first after mra_run, mra_run_resume, mra_sample or any set_*) runs one likelihood pass with W at every
 * row (MRA_OPT_LIK_ROWS overridden inside); later calls reuse the factors and launch only the solve kernels.  Afterwards y, every
 * option and what mra_get_likelihood / mra_get_predict return are as the caller left them (mra_get_timers / mra_get_kernel_stats
 * describe the call's own pass; all zero when none ran).  flags: 0 or MRA_SOLVE_FULL_QUAD.
 * MRA_SOLVE_FULL_QUAD: quad is the dense symmetric n_cols x n_cols matrix, no NaN.  Entries whose row and column share a block of 16
 * are bit for bit those of the call without the flag; the others come from k_solve_quad_cross: the forward sweep of every block
 * leaves its vectors (the leaves' U_y, the fronts' z: (sum nop + sum cw) x16 doubles per block, about 90 MB per block for a 1024^2
 * tree with r = 32) in an archive, and Q_ab = sum_seg sign F_a^T F_b is summed over a fixed number of partial sums in a fixed order
 * (the same bits on every call) and mirrored (symmetric to the bit).  At most MRA_FULL_QUAD_MAX columns (MRA_ERR_INVALID above,
 * checked before anything is launched).  The archive is allocated by flagged calls of more than 16 columns only (grow-only in the
 * number of blocks) and released when the solver's descriptors are rebuilt (new observations); a call without the flag allocates and
 * computes what it did before.
 * MRA_ERR_STATE before set_locs / set_obs / set_kernel; MRA_ERR_INVALID for unknown flags, MRA_KERNEL_HOST plans, sharded plans,
 * n_cols < 0 and a non-finite Y at an observed row.  Work buffers are allocated on the first call.  Blocking. */
#define MRA_SOLVE_FULL_QUAD 1u
#define MRA_FULL_QUAD_MAX 256
int mra_solve(mra_plan *plan, uint32_t flags, int64_t n_cols, const double *Y, double *mean, double *quad);

/* A regression trend (no counterpart in the reference, whose fields have mean zero): y_o = X_o beta + x_o + eps with a flat prior on
 * beta in R^p and K = Sigma_MRA[o, o] + D (D = R I, or the vector of mra_plan_set_noise).  With G = [y | X]^T K^-1 [y | X] (the full
 * quad of mra_solve for the columns [y | X]), G_yy = G[0][0], b = G[1:, 0], A = G[1:, 1:]:
 *     beta^ = A^-1 b, cov(beta^) = A^-1; profile -2 log-likelihood = d + (G_yy - b^T beta^); REML criterion = that + log det A
 * (d: the log-determinant of the pass, constants as in mra_get_likelihood), and with m_y, m_X the zero-mean kriging means of the
 * columns (mean of mra_solve), h(s) = x(s) - m_X(s): mean(s) = m_y(s) + h(s)^T beta^, var(s) = var_pass(s) + h(s)^T A^-1 h(s) - the
 * universal-kriging mean and variance (var_pass: the var of mra_get_predict after a predict pass on the plan's y).
 *
 * mra_plan_set_trend: X_perm is p x P, row-major (covariate j at X_perm + j P), padded leaf order, 0 at phantom rows; it is copied
 * to the device once and stays there: a property of the plan, as the noise vector is.  It survives mra_plan_set_obs*,
 * mra_plan_set_noise*, mra_plan_set_kernel, mra_plan_set_metric, mra_plan_set_locs* and every option, and it drops no factor (X
 * enters no factorisation).  p = 0 or X_perm = NULL with p = 0 clears it.  MRA_ERR_INVALID, checked on the host before anything
 * changes: p < 0, p > MRA_TREND_MAX, a NULL X_perm with p > 0, an entry of the p x P array that is not finite.  Works on
 * MRA_HOST_DRYRUN plans.  Memory: p P doubles on the device.
 *
 * mra_trend_fit: fits the trend to the plan's own y.  It shares the factors mra_solve keeps (one likelihood pass with W at every
 * row if they do not stand, none otherwise), stages [y | X] device to device in blocks of 16 columns (y with NaN read as 0, as
 * mra_solve reads Y: observed rows only), runs the forward sweeps and forms G as mra_solve with MRA_SOLVE_FULL_QUAD does (same
 * kernels, same archive: one panel per block, at most four), downloads G and factorises A = L L^T on the host.
 *     beta (p), cov_beta (p x p, or NULL)
 *     info[8]: [0] d; [1] G_yy - b^T beta^; [2] log det A; [3] the profile value [0] + [1]; [4] the REML value [3] + [2];
 *              [5] number of observed rows; [6] p; [7] min / max of diag(L)^2
 * With MRA_TREND_PREDICT the backward sweeps and the row kernel run per block, m_y and m_X stay on the device ((1 + p) P doubles,
 * allocated by the first such call, with 3 P more for var_pass and the results) and k_trend_rows writes
 *     mean_perm, var_perm (P each, padded leaf order, or NULL): the universal-kriging mean and variance; unreported rows exactly 0
 * var_pass comes from a predict pass on the plan's own y that the call runs itself (and keeps while the factors stand; the
 * likelihood pass for the factors follows it, since a predict pass rewrites W): the first predicting call runs two passes, later
 * calls none.  Afterwards y, every option and what mra_get_likelihood / mra_get_predict return are as the caller left them
 * (mra_get_timers / mra_get_kernel_stats describe the call's own last pass; all zero when none ran).
 * Refusals, in this order: those of every call on the retained factors (unknown flags: MRA_ERR_INVALID; before set_locs / set_kernel
 * / set_obs: MRA_ERR_STATE; MRA_KERNEL_HOST plans and sharded plans: MRA_ERR_INVALID); no trend set: MRA_ERR_STATE; a NULL beta or
 * info, mean_perm or var_perm without MRA_TREND_PREDICT: MRA_ERR_INVALID.  A pivot of A that is <= 0, NaN or below
 * p 2^-52 max diag(A): MRA_ERR_NOT_SPD, "trend columns are linearly dependent at the observed rows" (a host check of a matrix of at
 * most 63 x 63; beta is not written).  Blocking. */
#define MRA_TREND_MAX 63      /* [y | X] is at most 64 columns: four blocks */
#define MRA_TREND_PREDICT 1u
int mra_plan_set_trend(mra_plan *plan, int32_t p, const double *X_perm);
int mra_trend_fit(mra_plan *plan, uint32_t flags, double *beta, double *cov_beta, double *mean_perm, double *var_perm, double *info);

/* The two together: z_p ~ p(. | eta_p) with eta = X beta + x + offset, x ~ MRA(0, Sigma), a flat prior on beta
 * in R^p - the families, g, D, its floor and the starts of mra_plan_fit_laplace, X the resident matrix of mra_plan_set_trend.  The
 * iteration runs on e = eta - offset = X beta + x at the observed rows.  One iteration from e: t = e + g / D and r = 1 / D into the
 * plan's y and noise (the launch of mra_plan_fit_laplace); ONE likelihood pass with W at every row for the factors of K = Sigma_oo +
 * diag r (MRA_OPT_PRIOR_REUSE and MRA_OPT_RESID_REUSE hold from the second pass on: only the noise changed); the GLS step of
 * mra_trend_fit on [t | X] (same code: forward sweeps per block of 16 columns, cross tiles when p + 1 > 16, G to the host, A = L L^T,
 * beta^ = A^-1 b) with the backward sweeps and the row kernel per block, which leave the zero-mean kriging means m_t, m_X on the
 * device; and two launches (k_laplace_trend_part, k_laplace_sum) that form e^ = m_t + (X - m_X)^T beta^ = X beta^ + x^, make it the
 * iterate and return step = max |e^ - e| and the sums below (fixed partial results in a fixed order: the same inputs give the same
 * bits).  No predict pass runs.  The call stops after the pass with step <= tol * max(1, max |e^|), or after max_iter passes; a step
 * that is NaN or inf ends it, not converged.  Plain Newton, no damping.  The Gaussian family takes two passes, the second with step 0,
 * and its beta, cov_beta, info[0], [1], [8] are those of mra_trend_fit after mra_plan_set_obs(z - offset) + mra_plan_set_noise(aux).
 * z_perm, aux_perm, offset_perm as in mra_plan_fit_laplace; e0_perm: P values, the start of e (NULL: the data-based start of that
 * table, i.e. beta = 0 and x = that start).  beta (p), cov_beta (p x p = A^-1 of the last pass, or NULL).
 * info[12]: [0] d = log|K|; [1] G_tt - b^T beta^; [2] -2 sum log p(z_p | eta^_p), every constant included; [3] sum log D_p;
 * [4] sum D_p (t_p - e^_p)^2; [5] passes; [6] the last step; [7] converged; [8] log det A; [9] the profile value
 * -2 log q = [0] + [1] + [2] + [3] - [4] (beta at its mode); [10] the marginal value [9] + [8] - p log 2 pi (beta integrated out, the
 * Laplace REML criterion: the joint Hessian has det = det(Sigma^-1 + D) det A, and x^^T Sigma^-1 x^ = [1] - [4]); [11] the number
 * of observed rows.
 * Refusals, in this order, each checked on the host before anything changes: those of every call on the retained factors (before
 * set_locs / set_kernel / set_obs: MRA_ERR_STATE; MRA_KERNEL_HOST plans and sharded plans: MRA_ERR_INVALID); no trend set:
 * MRA_ERR_STATE; the argument checks of mra_plan_fit_laplace in its order (e0 in the place of x0); a NULL beta: MRA_ERR_INVALID.  On
 * MRA_HOST_DRYRUN plans all of these are reached, then MRA_ERR_STATE (the plan cannot run).  A pivot of A that fails mra_trend_fit's
 * test: MRA_ERR_NOT_SPD, "trend columns are linearly dependent at the observed rows", with that pass's t and r in the plan; a pass's
 * own MRA_ERR_NOT_SPD propagates likewise.
 * Afterwards the plan is a plan after mra_plan_set_obs(t) + mra_plan_set_noise(r) with the factors valid and the trend still set:
 * mra_trend_fit(MRA_TREND_PREDICT) gives the mean of e and its variance with the uncertainty of beta^ in it, mra_predict_sites,
 * mra_sites_cov and mra_solve serve the Laplace posterior, mra_get_buffer(10 / 11) give r / t.  What mra_get_likelihood /
 * mra_get_predict return stays as the caller left it, as after every call on the retained factors; mra_get_kernel_stats sums the
 * launches of the whole call (the new kernels under the family of the other elementwise ones), and mra_get_buffer(14) the stream
 * milliseconds of its sweeps as for mra_trend_fit, summed over the passes, the tail of the iterations under "rows".
 * mra_plan_fit_laplace itself ignores a trend.  Memory: as mra_trend_fit(MRA_TREND_PREDICT) without its 3 P.  Blocking. */
int mra_plan_fit_laplace_trend(mra_plan *plan, int family, const double *z_perm, const double *aux_perm, const double *offset_perm,
                               const double *e0_perm, int max_iter, double tol, double *beta, double *cov_beta, double *info);

/* The MRA covariance as an operator (no counterpart in the reference, which can only draw from it, pyMRA/MRATools.py:395-484): the
 * prior covariance of the latent field at the reported rows (real rows inside a leaf) is
 *     Sigma = sum over non-leaf j of W_j W_j^T + sum over leaves l of v_M(K_l, K_l),   v_M(S, S) = C(S, S) - W_anc[S] W_anc[S]^T,
 * W_j = W[rows of j, block of j's level], K_l the knot rows of leaf l - the Sigma mra_sample draws from.  For n_cols vectors A
 * (n_cols x P, row-major: vector k at A + k P, padded leaf order, read at the REPORTED rows only; values elsewhere are ignored)
 *     out  (n_cols x P, or NULL): out[k] = Sigma A[k]; with MRA_COV_POSTERIOR out[k] = Sigma_post A[k],
 *                                 Sigma_post = Sigma - Sigma[:, o] (Sigma[o, o] + D)^-1 Sigma[o, :] (D as in mra_solve) on the mask of the last set_obs, whose
 *                                 diagonal is the var of mra_get_predict; unreported rows (phantoms, rows a 1-D split drops) are exactly 0
 *     gram (n_cols x n_cols, or NULL): A Sigma A^T (A Sigma_post A^T), the covariance matrix of the functionals a_k^T x
 * Columns are processed in blocks of 16 (the N of v_mfma_f64_16x16x4_f64).  gram is returned BLOCK-DIAGONAL as quad of mra_solve is:
 * entries whose row and column lie in the same block of 16 columns are computed, all others are set to NaN.  It is summed over a fixed
 * number of partial sums in a fixed order (the same bits on every call) and returned symmetric.
 * The call shares the factors mra_solve keeps: the first call (and the first after mra_run, mra_run_resume, mra_sample or any set_*)
 * runs one likelihood pass with W at every row; later calls - and a later mra_solve, as this call after an mra_solve - launch no
 * factorisation.  Afterwards y, every option and what mra_get_likelihood / mra_get_predict return are as the caller left them
 * (mra_get_timers / mra_get_kernel_stats describe the call's own pass; all zero when none ran).
 * MRA_ERR_STATE before set_locs / set_obs / set_kernel; MRA_ERR_INVALID for unknown flags, MRA_KERNEL_HOST plans, sharded plans,
 * n_cols < 0, a NULL A with n_cols > 0 and a non-finite A at a reported row (checked on the host before anything is launched).
 * n_cols == 0 returns MRA_OK.  Work buffers are allocated on the first call.  Blocking. */
#define MRA_COV_POSTERIOR 1u
int mra_cov_apply(mra_plan *plan, uint32_t flags, int64_t n_cols, const double *A, double *out, double *gram);

/* Prediction at locations that are not rows of the tree (no counterpart in the reference, where a prediction location has to be a row
 * of `locs` with a NaN observation - which changes the knots and so the model, pyMRA/MRANode.py:36-45): the MRA is a process on the
 * whole domain, x(s) = sum_{m < lev(l)} a_m(s)^T eta_m + delta_l(s) for a site s assigned to leaf l, and the state mra_solve keeps
 * evaluates its posterior mean and variance anywhere:
 *     sites (n_sites x d, row-major, the caller's order) and leaf (the NODE index of the leaf each site is assigned to; any assignment
 *           gives a valid process, pymra_amd.MRATree.locate takes the leaf of the nearest tree location)
 *     Y     (n_cols x P as for mra_solve, read at the plan's OBSERVED rows only), or NULL: the plan's own observations, n_cols == 1
 *     mean  (n_cols x n_sites, or NULL): mean[k][i] = E[x(s_i) | Y[k] at the observed rows]
 *     var   (n_sites, or NULL): the posterior variance of the latent field at s_i (add R for a new observation); it does not depend on Y
 * At a site that is a tree location, assigned to that row's leaf, these are the mean and var of mra_get_predict.  Inside the library the
 * sites are grouped by leaf, each group is padded to tiles of 16 sites (the N of v_mfma_f64_16x16x4_f64) and the tiles are processed in
 * chunks of bounded work memory (MRA_OPT_SITES_CHUNK_BYTES); the result for a site is a pure function of (site, leaf, plan state) -
 * the same bits whatever else is in the call and however it is chunked.  Columns are processed in blocks of 16.
 * The call shares the factors mra_solve keeps: the first call (and the first after mra_run, mra_run_resume, mra_sample or any set_*)
 * runs one likelihood pass with W at every row; later calls - and calls after an mra_solve or mra_cov_apply - launch no factorisation.
 * Afterwards y, every option and what mra_get_likelihood / mra_get_predict return are as the caller left them (mra_get_timers /
 * mra_get_kernel_stats describe the call's own pass; all zero when none ran).  flags: 0.
 * MRA_ERR_STATE before set_locs / set_obs / set_kernel; MRA_ERR_INVALID for unknown flags, MRA_KERNEL_HOST plans, sharded plans,
 * n_sites < 0, n_cols < 0, a NULL sites or leaf with n_sites > 0, a leaf entry that is out of range or not a leaf node, a non-finite
 * site coordinate, a non-finite Y at an observed row and a NULL Y with n_cols != 1 (all checked on the host before anything is
 * launched).  n_sites == 0 returns MRA_OK.  Work buffers are allocated on the first call.  Blocking. */
int mra_predict_sites(mra_plan *plan, uint32_t flags, int64_t n_sites, const double *sites, const int32_t *leaf, int64_t n_cols,
                      const double *Y, double *mean, double *var);

/* The joint covariance of the latent MRA process at locations that are not rows of the tree (no counterpart in the reference; DESIGN.md
 * section 13): what mra_predict_sites gives the diagonal of.  With a_j(s), t(s) and p_j(s) of section 12 and l(u) the leaf of site u,
 *     prior      Sigma(u, w)      = C(s_u, s_w) if l(u) == l(w), else sum over the common ancestors j of a_j(u)^T a_j(w)
 *     posterior  Sigma_post(u, w) = sum over the common ancestors j of p_j(u)^T p_j(w)
 *                                   + [l(u) == l(w)] (C(s_u, s_w) - a(u)^T a(w) - t(u)^T t(w))
 *     sites, leaf as for mra_predict_sites; flags: 0 (prior) or MRA_COV_POSTERIOR (on the mask of the last set_obs)
 *     out   (n_sites x n_sites, row-major, the caller's order).  No entry is clamped: the posterior diagonal is mra_predict_sites' var
 *           without its max(., 0) on the leaf term, and the matrix is positive semi-definite down to roundoff only.
 * out is symmetric to the bit.  Entry (u, w) is a pure function of (site u, leaf u, site w, leaf w, plan state): the same bits whatever
 * else is in the call, in whatever order, and whatever MRA_OPT_SITES_CHUNK_BYTES says; duplicated sites give duplicated rows.  At sites
 * that are tree locations assigned to their own leaf the matrix is the corresponding block of mra_cov_apply's Sigma or Sigma_post, and
 * the posterior diagonal is the var of mra_get_predict up to rounding.  Inside the library the sites are tiled as for mra_predict_sites,
 * the work arrays of ALL tiles stay on the device for the call, and the matrix is produced in row panels of whole tiles (at least one;
 * MRA_OPT_SITES_CHUNK_BYTES bounds the device panel), each 16 x 16 block on or above the diagonal computed once and mirrored.
 * The state is mra_predict_sites': the first call (and the first after mra_run, mra_run_resume, mra_sample or any set_*) runs one
 * likelihood pass with W at every row; later calls - and calls after an mra_solve, mra_cov_apply or mra_predict_sites - launch no
 * factorisation.  Afterwards y, every option and what mra_get_likelihood / mra_get_predict return are as the caller left them.
 * MRA_ERR_STATE before set_locs / set_obs / set_kernel; MRA_ERR_INVALID for unknown flags, MRA_KERNEL_HOST plans, sharded plans,
 * n_sites < 0, n_sites > MRA_SITES_COV_MAX (the result is dense: 2 GiB at the cap), a NULL sites, leaf or out with n_sites > 0, a leaf
 * entry that is out of range or not a leaf node and a non-finite site coordinate (all checked on the host before anything is launched
 * or allocated).  n_sites == 0 returns MRA_OK.  Blocking. */
#define MRA_SITES_COV_MAX 16384
int mra_sites_cov(mra_plan *plan, uint32_t flags, int64_t n_sites, const double *sites, const int32_t *leaf, double *out);

/* Draws of the latent MRA process at locations that are not rows of the tree (no counterpart in the reference, which can only draw at
 * the rows of `locs`, pyMRA/MRATools.py:395-484).  Section 13's two covariance formulas are a factorisation
 * Sigma = F F^T with a sparse, tree-shaped F: with a_j(s), t(s), p_j(s) of section 12 and l(u) the leaf of site u,
 *     prior      x(s_u) =              sum over the chain j of l(u) of a_j(u)^T xi_j + (L_l zeta_l)_u,   L_l L_l^T = C(S_l, S_l) - a^T a
 *     posterior  x(s_u) = mean(s_u) +  sum over the chain j of l(u) of p_j(u)^T xi_j + (L_l zeta_l)_u,   L_l L_l^T = C - a^T a - t^T t
 * xi_j ~ N(0, I) one vector per non-leaf node, shared by every site below it; zeta_l ~ N(0, I) one entry per site of leaf l; S_l the
 * call's sites assigned to leaf l, in the caller's order (the order of the Cholesky); mean = mra_predict_sites' for the plan's own
 * observations.  The posterior draw needs no kriging pass: one basis / leaf / chain pass, one Cholesky per leaf that has sites, two
 * MFMA products per block of 16 samples.
 *     sites, leaf as for mra_predict_sites; flags: 0 (prior) or MRA_COV_POSTERIOR (on the mask of the last set_obs, mean included)
 *     out   (n_samples x n_sites, row-major, the caller's site order)
 *     latent slots [0, Kn): the non-leaf nodes, numbered exactly as mra_sample numbers them (node order, cw[level] each, knot-column
 *           order; phantom columns are inert: a and p are 0 there); [Kn, Kn + n_sites): the leaf term of site u, by the caller's index.
 *           mra_sample_sites_slots gives Kn + n_sites.
 *     z     NULL: Philox exactly as mra_sample draws (counter (slot, sample0 + s), key seed); else n_samples x n_slots, row-major
 * Samples go in blocks of 16 (the N of v_mfma_f64_16x16x4_f64).  Exact duplicates (same leaf, equal coordinates) are collapsed on the
 * host to their first occurrence: they receive its draw bit for bit, do not count towards MRA_SAMPLE_SITES_LEAF_MAX, and their own
 * leaf slots are not read.  A site with G_uu <= 2^-40 C(s_u, s_u) - it lies on a knot of an ancestor, its leaf term is structurally
 * zero - is inert: its row and column of G_l become the identity and its zeta is not used.
 * The coarse term and the mean of a site are a pure function of (site, leaf, plan state, seed, sample); the leaf term depends on the
 * call's sites in that leaf and their order and on nothing else in the call: the bits of out do not depend on
 * MRA_OPT_SITES_CHUNK_BYTES (which bounds a batch of whole leaves: work arrays + blocks, at least one leaf) nor on which other leaves
 * have sites.  Near-duplicate sites that make a pivot <= 0 give MRA_ERR_NOT_SPD naming the leaf; no jitter is added.
 * The state is mra_predict_sites': the first call (and the first after mra_run, mra_run_resume, mra_sample or any set_*) runs one
 * likelihood pass with W at every row; later calls - and calls after an mra_solve, mra_cov_apply, mra_predict_sites or mra_sites_cov -
 * launch no factorisation.  Afterwards y, every option and what mra_get_likelihood / mra_get_predict return are as the caller left them.
 * MRA_ERR_STATE before set_locs / set_obs / set_kernel; MRA_ERR_INVALID for unknown flags, MRA_KERNEL_HOST plans, sharded plans,
 * n_sites < 0, n_samples < 0, sample0 < 0 or a sample number past 2^63 - 1, a NULL out when there is something to write, a NULL sites
 * or leaf with n_sites > 0, a leaf entry that is out of range or not a leaf node, a non-finite site coordinate and a leaf that receives
 * more than MRA_SAMPLE_SITES_LEAF_MAX distinct sites (all checked on the host before anything is launched or allocated).
 * n_sites == 0 or n_samples == 0 returns MRA_OK.  Blocking. */
#define MRA_SAMPLE_SITES_LEAF_MAX 4096   /* distinct sites one leaf may receive in a call: its block is dense, 128 MiB at the cap */
int mra_sample_sites_slots(mra_plan *plan, int64_t n_sites, int64_t *n_slots);       /* Kn + n_sites */
int mra_sample_sites(mra_plan *plan, uint32_t flags, int64_t n_sites, const double *sites, const int32_t *leaf,
                     int64_t n_samples, uint64_t seed, int64_t sample0, const double *z, double *out);

/* Cross-validation of the fitted model from the retained factors, without a refit (no counterpart in the reference; DESIGN.md section
 * 18).  With o the observed rows, D = diag(r_o) the noise (the scalar R or the vector of mra_plan_set_noise), K = Sigma[o, o] + D, m and
 * Sigma_post the posterior mean and covariance of the latent field given all the data and rho = y - m: K^-1 = D^-1 - D^-1 Sigma_post D^-1
 * and K^-1 y = D^-1 rho, so for a group G of observed rows and N_G = D_G - Sigma_post[G, G] = L L^T the predictive distribution of y_G
 * given every observation OUTSIDE G is
 *     mean mu_G = y_G - D_G N_G^-1 rho_G,   covariance S_G = D_G N_G^-1 D_G (the noise of the new observation included),
 *     log N(y_G; mu_G, S_G) = -1/2 [2 sum log r_p - log det N_G + |L^-1 rho_G|^2 + |G| log 2 pi].
 * flags: 0 - leave one out, every observed row its own group: with h_p = v_p / r_p (v the posterior variance) mu_p = y_p -
 * rho_p / (1 - h_p) and S_pp = r_p / (1 - h_p); MRA_CV_LEAF - the groups are the observed rows of each leaf (spatial block
 * cross-validation on the tree's own partition), Sigma_post[G, G] by mra_sites_cov's same-leaf formula with the rows as sites.
 *     mean_perm, var_perm, lpd_perm   (P each, padded leaf order, any may be NULL): mu_p, S_pp - the predictive variance of a new y_p,
 *           noise included - and the marginal log N(y_p; mu_p, S_pp); NaN at rows the plan does not observe
 *     group_lpd   (n_nodes, or NULL): by leaf, the joint log predictive density of the group at its leaf's node index; otherwise the sum
 *           of that leaf's rows' lpd; NaN for non-leaves and for leaves without observations
 *     info[8]     0: rows scored; 1: groups; 2: the sum over groups of the joint log predictive density (the CV log score); 3: the sum
 *           over rows of the marginal lpd; 4: the sum of squared standardised residuals (y_p - mu_p)^2 / S_pp; 5: max_p h_p;
 *           6: tr K^-1 = sum (1 - h_p) / r_p; 7: alpha^T alpha = sum (rho_p / r_p)^2, alpha = K^-1 y.  [6] - [7] is the derivative of
 *           mra_get_likelihood's d + u with respect to tau for K + tau I at tau = 0: the exact derivative by the nugget.
 * CONDITIONING: the information sits in r - v, so float64 loses about eps / (1 - h)^2 whatever computes the identity: against
 * brute-force conditioning (dense, 60 points, groups of 12) the mean is off by 6e-15 max|y| at max h = 0.77, 2.5e-13 at 0.94, 3e-9 at
 * 0.9994 and 2e-5 at 0.99999 (diag S relatively: 9e-15, 1e-12, 1e-8, 2e-4).  info[5] reports max h so that a caller sees it.
 * The sums of info are folded over a fixed number of partial results in a fixed order: the same inputs give the same bits.  A row's
 * results are a pure function of (row, its group, plan state): they do not depend on MRA_OPT_SITES_CHUNK_BYTES (which bounds a batch
 * of whole leaves, at least one leaf).  A pivot of N_G that is <= 0 or NaN, or 1 - h_p <= 0 or NaN when every row is its own group,
 * gives MRA_ERR_NOT_SPD naming the leaf or the padded row; no jitter is added.  After mra_plan_fit_laplace the call scores what the plan
 * holds: the pseudo-observations t with noise 1 / D of the last linearisation (mra_get_buffer 11 and 10), not the counts.
 * The state is mra_predict_sites': the first call (and the first after mra_run, mra_run_resume, mra_sample or any set_*) runs one
 * likelihood pass with W at every row; later calls - and calls after an mra_solve, mra_cov_apply, mra_predict_sites, mra_sites_cov or
 * mra_sample_sites - launch no factorisation.  Afterwards y, every option and what mra_get_likelihood / mra_get_predict return are as
 * the caller left them.
 * MRA_ERR_STATE before set_locs / set_obs / set_kernel; MRA_ERR_INVALID for unknown flags, MRA_KERNEL_HOST plans, sharded plans, a NULL
 * info, a noise variance that is 0 at an observed row and, by leaf, a leaf with more than MRA_SAMPLE_SITES_LEAF_MAX observed rows (all
 * checked on the host before anything is launched or allocated).  A plan with no observed row returns MRA_OK with info all zero.
 * Blocking. */
#define MRA_CV_LEAF 1u   /* groups = the observed rows of each leaf; 0: every observed row its own group */
int mra_cv(mra_plan *plan, uint32_t flags, double *mean_perm, double *var_perm, double *lpd_perm, double *group_lpd, double *info);

/* mra_cv for a plan with a regression trend (mra_plan_set_trend): the model is y = X beta + x + eps with a flat
 * prior on beta, as in mra_trend_fit.  With A = X^T K^-1 X = L_A L_A^T, m_y / m_X the kriging means of y and of the columns of X,
 * h_p = X_p - m_X(p), w_p = L_A^-1 h_p, rho~_p = y_p - m_y(p) - h_p^T beta^ (y minus the universal-kriging mean) and W_G the rows w_p^T:
 * P = K^-1 - K^-1 X A^-1 X^T K^-1 has P y = D^-1 rho~ and P[G, G] = D_G^-1 (N_G - W_G W_G^T) D_G^-1.
 * flags: MRA_CV_LEAF as in mra_cv, and
 *   MRA_CV_TREND_REFIT - beta is estimated again without the left-out group (universal-kriging cross-validation): mra_cv's formulas
 *     with rho~ for rho and N~_G = N_G - W_G W_G^T for N_G; by row h~_p = (v_p + |w_p|^2) / r_p, mu_p = y_p - rho~_p / (1 - h~_p),
 *     S_pp = r_p / (1 - h~_p).  X without the group's rows must keep full column rank, otherwise N~_G is singular;
 *   without it the beta^ of the full fit is plugged in: rho~ with the plain N_G, which is mra_cv on y - X beta^ reported on the scale
 *     of y.
 * The outputs are mra_cv's.  info[12]: 0 .. 4 as mra_cv; 5: the largest leverage the mode divides by (h~ with MRA_CV_TREND_REFIT, else
 * v / r); 6: tr K^-1 = sum (1 - v_p / r_p) / r_p; 7: |P y|^2 = sum (rho~_p / r_p)^2; 8: tr P = sum (1 - (v_p + |w_p|^2) / r_p) / r_p;
 * 9: p; 10: [6] - [7], the exact derivative of the profile -2 log L (mra_trend_fit's info[3]) by a nugget added to every observed row;
 * 11: [8] - [7], that of the REML criterion (info[4]).  The sums are folded over a fixed number of partial results in a fixed order:
 * the same inputs give the same bits, whatever MRA_OPT_SITES_CHUNK_BYTES is.
 * The call first fits the trend on the plan's own y as mra_trend_fit does, with the backward sweeps but without the predict pass of
 * MRA_TREND_PREDICT (1 + p right-hand sides in blocks of 16; no factorisation when the factors stand), then runs mra_cv's batches
 * with two more kernels.  Afterwards y, the options, what mra_get_likelihood / mra_get_predict return and what mra_trend_fit and mra_cv
 * return are as before.  After mra_plan_fit_laplace_trend the call scores what the plan holds: t, 1 / D and X.
 * Refusals: mra_cv's, in its order, with MRA_ERR_STATE when no trend is set right after the plan's own checks; on MRA_HOST_DRYRUN plans
 * all of these are reached, then MRA_ERR_STATE (the plan cannot run).  The trend fit's MRA_ERR_NOT_SPD ("trend columns are linearly
 * dependent at the observed rows") comes before any cross-validation kernel is launched.  With MRA_CV_TREND_REFIT a pivot of N~_G that
 * is <= 0 or NaN, or 1 - h~_p <= 0 or NaN, gives MRA_ERR_NOT_SPD naming the leaf or the padded row: the group may carry the only
 * information on a covariate.  That test is best effort - a rank loss in exact arithmetic can leave a tiny positive pivot in floating
 * point, and then the results of that group are meaningless; info[5] close to 1 is the sign to look for.
 * Memory beyond mra_cv's: (1 + p) P doubles for the means, P for |w|^2, and 16 (p rounded up to 4) doubles per tile of a batch (counted
 * against MRA_OPT_SITES_CHUNK_BYTES).  mra_get_buffer(15) gives the stream milliseconds of the call.  Blocking. */
#define MRA_CV_TREND_REFIT 2u        /* with MRA_CV_LEAF = 1u; without it beta^ is held fixed */
int mra_cv_trend(mra_plan *plan, uint32_t flags, double *mean_perm, double *var_perm, double *lpd_perm, double *group_lpd, double *info /* 12 */);

/* Diagnostics for tests (the reference exposes these as attributes of Node objects):
 * what = 0: whitened basis W (P x ldw, row-major) ; 1: per-node log-det terms (n_nodes);
 * 7: stream milliseconds of the last mra_predict_sites, measured while MRA_OPT_KERNEL_TIMING is on (7 values: the basis, leaf, chain
 * and mean kernels, the solver's sweeps, the uploads of sites and the downloads of results);
 * 8: the same for the last mra_sites_cov (6 values: the basis, leaf, chain and gram kernels, the uploads and the downloads);
 * 9: the same for the last mra_sample_sites (9 values: basis, leaf, chain, leaf Gram, leaf Cholesky, draw, mean with the solver's
 * sweeps, uploads, downloads);
 * 10: the noise variance by padded row (P values): the vector of mra_plan_set_noise at observed rows and 0 elsewhere, or the scalar R
 * at every row when no vector is set;
 * 11: the observations y by padded row as the device holds them (P values, NaN where nothing is observed): what the last
 * mra_plan_set_obs uploaded, or the pseudo-observations t of the last pass of mra_plan_fit_laplace;
 * 12: stream milliseconds of the last mra_cv under MRA_OPT_KERNEL_TIMING (9 values: basis, leaf, chain, mean with the solver's sweeps,
 * Gram, Cholesky, solve with the reduction, uploads, downloads);
 * 13: the coordinates as the kernels read them (P x d, padded leaf order): what mra_plan_set_locs uploaded, or A x under
 * mra_plan_set_metric;
 * 14: the last mra_trend_fit (7 values): stream milliseconds under MRA_OPT_KERNEL_TIMING (0 without) of the device-to-device staging
 * of [y | X], of the solver's sweeps of all blocks with the diagonal tiles of G and the archive copies, of k_solve_quad_cross with its
 * fold, of k_trend_rows, and of the uploads and downloads; then the bytes of the leaves' Ut (a forward sweep reads them once per
 * block) and of one block's archive panel (written once, read once);
 * 15: stream milliseconds of the last mra_cv_trend under MRA_OPT_KERNEL_TIMING (12 values: the nine of 12, then the trend's sweeps
 * with their staging and transfers, k_cv_trend, k_cv_downdate);
 * 16: the quadrature table of an MRA_KERNEL_MATERN plan as the device holds it (191 pairs (cosh(k h), c h cosh(nu k h)), h = 0.2,
 * c = 2^(1-nu) / Gamma(nu), the weight halved at k = 0; 0 values while the plan has another kernel);
 * 17: the component table of an MRA_KERNEL_SUM plan as the device holds it (K records {submode, c / l, 1 / (2 l^2), a1, a2, scale sig_c},
 * then one value more, C(x, x) = the sum of the records' last entries as the kernels are handed it; 0 values while the plan has another kernel);
 * copies min(capacity, available) doubles into out, returns the available count in *n_avail.
 * (W after a likelihood-only run is complete only with MRA_OPT_LIK_ROWS off: by default such a run computes W at the rows a
 * likelihood needs - the observed rows, and the knots on the level-by-level path - and leaves the others as they were.) */
int mra_get_buffer(mra_plan *plan, int what, double *out, int64_t capacity, int64_t *n_avail);

/* Diagnostics for tests: the route of the last pass - WHICH kernels it launched ("How a pass chooses its
 * kernels"; PassRoute in mra_plan_types.h).  An accepted option is not yet a kernel that ran: thresholds on the tree (largest leaf
 * in observation tiles, leaves per CU, block widths) override options, and this call shows the outcome.  It reads what mra_run
 * (or the pass inside mra_sample / mra_solve) fixed when the pass opened and changes nothing.  out[k], k < min(capacity,
 * MRA_ROUTE_FIELDS), in this order (booleans as 0 / 1):
 *    0 path (MRA_ROUTE_PATH_*)   1 predict        2 init_yblock    3 acc_var        4 n_chain       5 prior_level    6 c_only
 *    7 lik_rows                  8 lik_general    9 scatter_ut    10 leaf_resident 11 c_fix (MRA_ROUTE_CFIX_*)
 *   12 chol (MRA_ROUTE_CHOL_*)  13 var (MRA_ROUTE_VAR_*)          14 update (MRA_ROUTE_UPDATE_*)   15 solve_fused
 *   16 direct_parent            17 parent_front  18 front_fused   19 syrk_blk      20 syrk_dma     21 side          22 extract_mean
 *   23 n_leaves   24 n_trsm_small (leaves of at most 8 observation tiles: first in the fused path's row-solve and update lists)
 *   25 n_chol_small (the same count for the split k_chol_tiles launch)   26 n_cu (compute units the thresholds count leaves against)
 * Returns the number of fields written, MRA_ERR_STATE before the first pass, MRA_ERR_INVALID for a NULL argument. */
#define MRA_ROUTE_FIELDS            27
#define MRA_ROUTE_PATH_FUSED         0   /* regular tree: one-kernel cascades                                         */
#define MRA_ROUTE_PATH_HI            1   /* deep 64-wide tree: level-by-level prior and fronts, k_predict_hi          */
#define MRA_ROUTE_PATH_LEVELS        2   /* level-by-level kernels                                                    */
#define MRA_ROUTE_CFIX_NONE          0   /* no leaf has an observation                                                */
#define MRA_ROUTE_CFIX_IN_PRODUCT    1   /* likelihood-only: the gathered COV product wrote all of C                  */
#define MRA_ROUTE_CFIX_PHANTOM       2   /* k_leaf_cphantom                                                           */
#define MRA_ROUTE_CFIX_FILL          3   /* k_leaf_fill (a leaf of more than 192 observations)                        */
#define MRA_ROUTE_CHOL_TILES_ONE     0   /* k_chol_tiles<10,4> for every leaf                                         */
#define MRA_ROUTE_CHOL_TILES_SPLIT   1   /* k_chol_tiles<8,4> for the n_chol_small leaves, <10,4> for the others      */
#define MRA_ROUTE_CHOL_WAVE          2   /* k_chol_wave                                                               */
#define MRA_ROUTE_CHOL_BIG_PANELS    3   /* right-looking panels + trailing GEMM                                      */
#define MRA_ROUTE_VAR_NONE           0   /* the predictive cascade's own (or no predict pass)                         */
#define MRA_ROUTE_VAR_FINISH_VAR     1   /* accumulated by the row solves, k_leaf_finish_var                          */
#define MRA_ROUTE_VAR_MOMENTS        2   /* k_leaf_moments                                                            */
#define MRA_ROUTE_UPDATE_NONE        0   /* no predict pass                                                           */
#define MRA_ROUTE_UPDATE_IN_CASCADE  1   /* in k_predict_cascade (leaves of more than 8 observation tiles: GEMM)      */
#define MRA_ROUTE_UPDATE_IN_PREDICT_HI 2 /* in k_predict_hi                                                           */
#define MRA_ROUTE_UPDATE_SOLVE_WHOLE 3   /* k_leaf_solve_update, one workgroup per leaf (larger leaves: GEMM)         */
#define MRA_ROUTE_UPDATE_SOLVE_HALVES 4  /* k_leaf_solve_update, two workgroups per leaf (larger leaves: GEMM)        */
#define MRA_ROUTE_UPDATE_GEMM        5   /* k_gemm_nt_lds<SUB>                                                        */
#define MRA_ROUTE_UPDATE_LEAF_GEMM   6   /* k_leaf_gemm<SUB>                                                          */
int mra_get_route(mra_plan *plan, int32_t *out, int capacity);

/* Replaces: the per-node attributes the reference leaves on its Node objects - B, kInv (pyMRA/MRANode.py:384-385),
 * kTil, A, omg (:426-445), BTil (:486-495) - which its diagnostics read (MRATree.getBasisFunctionsMatrix,
 * pyMRA/MRATree.py:445-511; pyMRA/tests/debug-posterior.py:97-109).  The device keeps them in whitened form
 * (DESIGN.md section 3); this call copies one node's raw block, pymra_amd.diagnostics de-whitens on the host:
 *   MRA_BLOCK_W_ROWS  the node's rows of the whitened basis array W, all ldw columns (N_j x ldw).  After a
 *                     likelihood-only run (MRA_OPT_LIK_ROWS off): the prior W (B_k[S_j] = W[:, block k] L_k^T).  After a predict run with
 *                     MRA_OPT_FUSED off: block m of a level-m non-leaf node's rows holds X = BTil_j[m] (L_j Lt_j)^-T
 *                     (X X^T = BTil[m] kTil BTil[m]^T), the blocks of coarser levels hold the rows of BTil[k] L_k^-T
 *                     as the node's parent sees them.
 *   MRA_BLOCK_LPRIOR  non-leaf: L_j, cw x cw lower Cholesky factor of kInv_j (padded with the identity)
 *   MRA_BLOCK_FRONT   non-leaf: the factorised front, nf x nf (lower triangle): Lt_j (cw x cw), Zt_j below it
 *                     (na x cw), the Schur block Gt_j (na x na) - whitened ATil / omgTil / u (last block = y)
 *   MRA_BLOCK_LEAF    leaf: the panel [C = v_m(o,o) + R I (diag(r_o) with mra_plan_set_noise) -> Lc ; Ut ; Tt], (nop + na + N_j) x nop
 *                     (Lc: the lower triangle; what stands above it is not defined - a pass that reads C from the kept
 *                     residual, MRA_OPT_RESID_REUSE, never writes there)
 * out receives min(capacity, rows*cols) doubles row-major; *n_rows, *n_cols the block shape. */
#define MRA_BLOCK_W_ROWS   0
#define MRA_BLOCK_LPRIOR   1
#define MRA_BLOCK_FRONT    2
#define MRA_BLOCK_LEAF     3
int mra_get_node_block(mra_plan *plan, int32_t node, int what, double *out, int64_t capacity,
                       int64_t *n_rows, int64_t *n_cols);

/* Device blocks of destroyed plans are cached per (device, size) and reused by later plans of the process - the reference's
 * MLE pattern builds a new MRATree per objective call (README.md:96-104).  This hands every cached block back to the driver. */
int mra_release_cached_memory(void);

/* Caller-order variants of mra_plan_set_locs / mra_plan_set_obs / mra_get_predict: the arrays are in the CALLER's row order
 * (locs N x d, y N; NaN = missing), src[P] / perm[P] / in_leaf[P] are the topology's row maps (padded row -> caller row it
 * copies; -1 in perm for a phantom row; in_leaf = row is reported).  The gather / scatter runs inside the library (threads +
 * a pinned staging area), which is what an end-to-end MRATree(...) call pays for instead of NumPy fancy indexing and
 * pageable copies (MRATree.__init__, pyMRA/MRATree.py:61-69, hands the arrays over in caller order). */
int mra_plan_set_locs_rows(mra_plan *plan, const double *locs, const int64_t *src);
int mra_plan_set_obs_rows(mra_plan *plan, const double *y, const int64_t *src, const int64_t *perm, double R);
int mra_get_predict_rows(mra_plan *plan, const int64_t *perm, const uint8_t *in_leaf, int64_t N, double *mean, double *var);
/* The same with sd = sqrt(var) written beside it (MRATree.predict returns np.sqrt(root.var), pyMRA/MRATree.py:93); sd may be NULL. */
int mra_get_predict_rows_sd(mra_plan *plan, const int64_t *perm, const uint8_t *in_leaf, int64_t N, double *mean, double *var,
                            double *sd);

/* Per-phase device milliseconds of the last mra_run (hipEvent deltas on the plan's stream):
 * out[0]=prior, [1]=leaf, [2]=fronts, [3]=predict, [4]=total; returns how many were written.
 * The four phase entries are measured only while MRA_OPT_KERNEL_TIMING is on (0 otherwise): an event
 * between dependent launches costs a few microseconds of stream time; the total is always measured. */
int mra_get_timers(mra_plan *plan, double *out_ms, int capacity);

/* Kernel-level timing: with option MRA_OPT_KERNEL_TIMING on, every launch of mra_run is bracketed by
 * hipEvents on the plan's stream; afterwards mra_get_kernel_stats reports, per kernel family
 * (0 .. mra_kernel_family_count()-1), its name, the number of launches, their summed device
 * milliseconds and the algorithmic flop count of those launches. */
#define MRA_OPT_KERNEL_TIMING  1
#define MRA_OPT_GEMM_LDS       3   /* 1 (default): LDS-tiled batched GEMM; 0: direct-load variant */
#define MRA_OPT_FUSED          2   /* 1 (default): fused cascade kernels on regular trees; 0: level-by-level kernels */
#define MRA_OPT_KNOT_CHAIN     5   /* 1 (default): knot pass of all levels in one launch (k_knot_chain); 0: one launch per level */
#define MRA_OPT_LEAF_GEMM      6   /* 1 (default): leaf-resident residual product (k_leaf_gemm, one workgroup per leaf); 2: also the leaf
                                      update; 0: 64x64-tile k_gemm_nt_lds for both */
#define MRA_OPT_LEAF_SOLVE     7   /* row solve Tt = V Lc^-T and leaf update in one launch (k_leaf_solve_update, Tt stays in registers):
                                      2 (default) when a CU sees at most two leaves (8-way sharded runs), 1 always, 0 never */
#define MRA_OPT_PRED_UPDATE    8   /* 1 (default): the leaf update is applied inside the predictive cascade (W is not rewritten); 0: separate product */
#define MRA_OPT_LEAF_SOLVE_SPLIT 10 /* 2 (default): the fused row solve + update runs two workgroups per leaf (half the row tiles each), so that
                                      the side stream frees CUs sooner for the front chain; 1: one workgroup per leaf */
#define MRA_OPT_CHOL_TILES     11  /* leaf Cholesky by one workgroup per matrix with the tiles in registers (k_chol_tiles): 1 (default) when a CU sees
                                      at most two leaves of at most 160 observations (sharded runs), 2 always, 0 never (one wave per matrix, k_chol_wave) */
#define MRA_OPT_SEG_GEMM_LDS   12  /* 1 (default): the panel columns of the leaves' parents (a segmented product: sum over the children's Ut blocks; deep
                                      64-wide trees) run on the LDS-tiled GEMM; 0: on the direct-load GEMM */
#define MRA_OPT_UT_GATHER      13  /* 1 (default): the leaves' Ut = [W_anc[o] | y_o]^T is gathered from W by the row solve (128-byte segments); 0: scattered
                                      by the prior row cascade in 8-byte pieces (the round-2 path: 0.02 ms slower per C3 pass) */
#define MRA_OPT_FRONT_FUSED    4   /* 1 (default): one LDS-resident launch per front level; 0: assemble / Cholesky / Schur launches */
#define MRA_OPT_SYRK_BLK       14  /* 1 (default): the grandparents' signed segmented SYRK of deep 64-wide trees on 96 x 96 blocks through LDS,
                                      the stage filled by LDS DMA (k_syrk_dma); 2: through registers (k_syrk_blk); 0: 32 x 32 wave tiles (k_gemm_nt) */
#define MRA_OPT_PRIOR_LEVEL    15  /* 1 (default): level-by-level path, blocks <= 64 wide: the prior of a level in one launch (residual product,
                                      kernel, row solve; the knots' block straight into its factor); 0: four launches per level */
#define MRA_OPT_HI_FOLD        16  /* 1 (default): deep 64-wide trees on one GPU: the leaf update W -= Tt Ut^T inside k_predict_hi (leaves of at most
                                      64 padded observations); 0: a product of its own over all of W; 2: inside k_predict_hi on a sharded rank too */
#define MRA_OPT_LIK_ROWS       17  /* 1 (default): likelihood-only passes of the fused path compute the whitened basis W at the OBSERVED rows only
                                      (gathered row tiles: a likelihood needs nothing else; W's other rows keep what an earlier pass left there);
                                      0: at every row - what mra_get_buffer(W) callers and the node-block diagnostics want */
#define MRA_OPT_CASCADE_GROUP  18  /* fused path, row cascades that stage all their levels at once: 1 = one workgroup per family of sibling
                                      leaves (one operand image staged for all of them), 0 = one per leaf.  Default: a cost model at plan build
                                      (families when that still fills the CUs); get returns the plan's current decision, set forces it.  Regular trees
                                      only: on any other plan set is accepted and ignored, get returns 0 */
#define MRA_OPT_SAMPLE_GRAM_BYTES 19 /* mra_sample: bytes of leaf Gram blocks (+ inverted diagonal blocks) per factorisation batch, at least one
                                      leaf per batch; 0 (default): 1.5 GB.  A new value drops the sampler's index maps and buffers, which
                                      the next mra_sample rebuilds.  The draws do not depend on it. */
#define MRA_OPT_SAMPLE_SOLVE   20  /* mra_sample with MRA_SAMPLE_CONDITIONAL: 0 (default): one likelihood + predict pass per draw; 1: the pseudo-data of
                                      a block of up to 16 draws are 16 right-hand sides of mra_solve's sweeps over the factors of the
                                      block's prior pass (one pass per block instead of 1 + 16) */
#define MRA_OPT_SITES_CHUNK_BYTES 21 /* mra_predict_sites: bytes of site work buffers (a, b, t, sites, results) per chunk of tiles, at least one tile
                                      per chunk; mra_sites_cov: bytes of the device row panel of its result, at least one tile row per panel.
                                      0 (default): 256 MiB.  The results do not depend on it; setting it keeps mra_solve's factors */
#define MRA_OPT_LEAF_ORDER     22  /* scheduling of the per-leaf launches of the fused path; the results do not depend on it, bit for bit.
                                      1 (default): (a) where the leaf Cholesky is split in two launches, the few leaves of more than 8 observation
                                      tiles factorise, solve and (predict) update on the side stream beside the small ones; (b) inside the small
                                      leaves and inside the others, every ordered leaf list takes the leaves of most tiles first.  0: leaf order,
                                      serial launches.  For A/B runs: 2: (a) alone, 3: (b) alone, 4: 1 with the residual product's problems in
                                      that order as well.  (a) is read when a pass opens; (b) when the leaf lists are built: it takes effect
                                      with the next mra_plan_set_obs.  mra_get_route does not report it */
#define MRA_OPT_PARENT_PAIR    23  /* which kernel factorises the fronts of the leaves' parents (k_parent_front's step of a pass); the results do
                                      not depend on it, bit for bit.  1 (default): k_parent_front_pair - four-wave workgroups, two to a CU - where
                                      the fronts fit it (at most 92 tiles, 64 KB of LDS) and the level has more fronts than the device has CUs;
                                      0: always k_parent_front (eight waves, one workgroup per CU); 2: the pair kernel wherever the fronts fit
                                      (tests, A/B runs).  Read at every launch.  mra_get_route does not report it */
#define MRA_OPT_PRIOR_REUSE    24  /* fused path: a pass that follows one with the same kernel, locations and knots keeps that pass's prior - the
                                      levels' factors and, where they were written at the rows it needs, the rows of W and the prior variance -
                                      and launches neither prior kernel: it writes W's y block again, puts the prior variance back and re-runs the
                                      row cascade on the few leaves whose rows the last update rewrote.  The results do not depend on it, bit for
                                      bit.  1 (default); 0: every pass computes its prior, the launches are those of a plan's first pass.  Every
                                      mra_plan_set_kernel / set_locs / set_cov_block / set_reduce_level, every option but 1, 20 and 21, and a pass
                                      that fails drop what is kept; mra_plan_set_obs and set_noise do not.  mra_get_route does not report it */
#define MRA_OPT_RESID_REUSE    25  /* fused path, k_chol_tiles routes with the Ut rows gathered: the leaves' residual V[S,o] and v(o,o) - which
                                      depend on the kernel, the locations, the knots and the mask, not on y, R or a noise vector - go to a buffer
                                      of the plan's own beside the panels (sum over the leaves of (n_obs16 + N_j) n_obs16 doubles, 1.35 GB at config
                                      c3, allocated by the first such pass; a refused allocation only means that nothing is kept).  The Cholesky and
                                      the row solves read it and store where they always did, so a pass that keeps its prior (option 24) on the
                                      same mask launches no residual product.  Bit-identical results.  1 (default); 0: the in-place launch list.
                                      Dropped with the prior, and by a mra_plan_set_obs whose mask differs.  mra_get_route does not report it */
int mra_plan_set_option(mra_plan *plan, int option, int64_t value);
/* current value of an option (so that a caller can change one temporarily and put it back) */
int mra_plan_get_option(mra_plan *plan, int option, int64_t *value);
/* Raise the dynamic-LDS limit (160 KB) of every kernel the plan may launch on the plan's own device now rather than at
 * first launch.  The attribute is per kernel AND per device, so it is recorded per plan: two MRATree objects on two
 * devices of one process each take this path.  *n_kernels (may be NULL): kernels on record for this plan. */
int mra_plan_prepare(mra_plan *plan, int64_t *n_kernels);
int mra_kernel_family_count(void);
int mra_get_kernel_stats(mra_plan *plan, int which, char *name, int name_cap, int *launches, double *ms,
                         double *flops);
/* Work of the family's launches in the last mra_run: out[0] algorithmic flops (true ranks, true observation counts, one y
 * column), out[1] flops the MFMA tiles execute on the 16-padded layout, out[2] algorithmic HBM bytes (every operand array of
 * the launch read or written once), out[3] summed device milliseconds (as mra_get_kernel_stats). */
int mra_get_kernel_work(mra_plan *plan, int which, double *out, int capacity);
/* hipDeviceSynchronize on `device` (bench.py's barrier: the timed region needs no second GPU runtime in the process) */
int mra_device_synchronize(int device);
/* out[0..9] = P, ldw, Ka, n_leaves, bytes(W), bytes(leaf panels), bytes(leaf Gt), n_nodes, p of mra_plan_set_trend (0: none),
 * bytes(resident design matrix) */
int mra_plan_info(mra_plan *plan, int64_t *out, int capacity);

/* ---- native host tree replay (no GPU involved) -------------------------------------------------------
 * Replaces, for large 2-D trees (every node above the leaves has > 100 rows and > 100 candidates, J = 4): the
 * knot selection and partition part of Node.__init__ (pyMRA/MRANode.py:34-59, 191-193, 232-239) and the flat
 * layout of pymra_amd.topology.  mt_key[624] / mt_pos are NumPy's global MT19937 state
 * (np.random.get_state()[1:3]); on success they hold the state after the reference's knot draws.
 * Returns 0, or 1 when the tree does not follow those rules (state untouched; use the Python replay). */
typedef struct mra_tree mra_tree;
int mra_tree_replay_2d(const double *locs, int64_t N, int32_t r, int32_t M, uint32_t *mt_key, int32_t *mt_pos,
                       mra_tree **out);
/* The same replay writing the four long arrays (perm, src, in_leaf: P <= cap_rows entries; knot_rows: N entries) straight into
 * caller buffers of capacity cap_rows >= N + 15 * 4^M (every leaf is padded to a multiple of 16 rows); mra_tree_export then
 * skips them (pass NULL).  Saves ~25 MB of copies and unmapping per tree: an end-to-end MRATree(...) call is mostly this. */
int mra_tree_replay_2d_into(const double *locs, int64_t N, int32_t r, int32_t M, uint32_t *mt_key, int32_t *mt_pos,
                            int64_t cap_rows, int64_t *perm, int64_t *src, uint8_t *in_leaf, int64_t *knot_rows,
                            mra_tree **out);
/* MRATree.__init__ for large 2-D trees in ONE call (pyMRA/MRATree.py:61-69 -> Node.__init__, MRANode.py:23-115): the replay
 * of mra_tree_replay_2d_into AND mra_plan_create + mra_plan_set_locs_rows + mra_plan_set_obs_rows, overlapped - the plan is sized,
 * allocated and fed its locations (locs: the caller's N x 2 rows) and observations (y: N values, NaN = missing; R: nugget) on a
 * helper thread while the calling thread draws the knots.  On success *tree_out is the tree (mra_tree_sizes / mra_tree_export /
 * mra_tree_free as usual; perm, src, in_leaf, knot_rows are written to the caller's buffers) and *plan_out a plan that only
 * needs mra_plan_set_kernel before mra_run.  Returns 1 - nothing created, RNG state untouched - when the tree does not follow
 * the large-2-D rules (use mra_tree_replay / the Python replay and mra_plan_create then), < 0 on errors. */
int mra_plan_create_replay_2d(const double *locs, int64_t N, int32_t r, int32_t M, uint32_t *mt_key, int32_t *mt_pos,
                              const double *y, double R, int device, int64_t cap_rows,
                              int64_t *perm, int64_t *src, uint8_t *in_leaf, int64_t *knot_rows,
                              mra_tree **tree_out, mra_plan **plan_out);
/* out5 = {P, n_nodes, n_levels, len(child_list), len(knot_rows)} */
int mra_tree_sizes(mra_tree *t, int64_t *out5);
/* copies the arrays of `mra_topology` (+ perm, src, in_leaf, node_level, pre-order) into caller buffers */
int mra_tree_export(mra_tree *t, int64_t *perm, int64_t *src, uint8_t *in_leaf, int64_t *level_ptr,
                    int32_t *node_level, int64_t *row0, int64_t *row1, uint8_t *leaf, int32_t *parent,
                    int32_t *child_ptr, int32_t *child_list, int64_t *knot_ptr, int64_t *knot_rows, int32_t *cw,
                    int32_t *preorder);
int mra_tree_free(mra_tree *t);

/* ---- multi-GPU: one process per GPU, subtrees sharded, ONE all-reduce of the shard-level fronts --
 * The reference's only parallel mode forks one process per child subtree at `critDepth` and pickles
 * the finished Node back (pyMRA/MRANode.py:64-65, 90-104, 114-115); here each rank owns whole
 * subtrees and the level above them is summed with one ncclAllReduce over xGMI.               */
int mra_comm_unique_id(char *out, int capacity);                 /* 128 bytes; rank 0 calls, then broadcast */
int mra_comm_init(mra_plan *plan, const char *unique_id, int n_ranks, int rank);
/* reduce_level: nodes of this level get their assembled fronts summed over ranks before they are
 * factorised (-1: no reduction). */
int mra_plan_set_reduce_level(mra_plan *plan, int level);

/* Front exchange without RCCL (tests on one GPU, or another transport): mra_run stops before the
 * reduce level's factorisation when MRA_RUN_SPLIT is set in flags; export/import the summed
 * fronts, then call mra_run_resume.  The resumed half runs the route (which kernels, in which
 * order) fixed by that mra_run: an option set in between takes effect with the next mra_run. */
#define MRA_RUN_SPLIT          4u
int mra_reduce_size(mra_plan *plan, int64_t *n_doubles);
int mra_reduce_export(mra_plan *plan, double *out);
int mra_reduce_import(mra_plan *plan, const double *in);
int mra_run_resume(mra_plan *plan);

const char *mra_last_error(mra_plan *plan);   /* plan may be NULL: last create error */
const char *mra_version(void);

#ifdef __cplusplus
}
#endif
#endif
