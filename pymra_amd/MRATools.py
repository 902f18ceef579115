"""Covariance plug-ins, distances and grid generators with the reference's call surface.

Mirrors the part of pyMRA/MRATools.py that the inference path and its callers use:

* ``dist``              pyMRA/MRATools.py:229-245
* ``Iden``              pyMRA/MRATools.py:256-262
* ``ExpCovFun``         pyMRA/MRATools.py:265-269
* ``Matern52``          pyMRA/MRATools.py:281-285
* ``Matern32``          pyMRA/MRATools.py:289-293
* ``GaussianCovFun``    pyMRA/MRATools.py:297-301
* ``Matern``            pyMRA/MRATools.py:273-277 (there through sklearn's ``Matern(nu=...)``; here with ``locs2``)
* ``genLocations``      pyMRA/MRATools.py:180-187
* ``genLocations2d``    pyMRA/MRATools.py:192-203

Each kernel keeps the reference's signature and, for array inputs, its ``np.matrix`` result.
The device path adds one thing: when a kernel is called with the *symbolic* location handles
that ``MRATree`` uses to probe a user's ``cov`` callable, it returns a ``KernelSpec`` (kind +
parameters, closed under multiplication by a scalar such as ``sigma*mt.Matern32(...)``,
cf. pyMRA/tests/test-param-est.py:84) instead of numbers; ``MRATree`` then evaluates that
kernel on the GPU.  Specs add: ``mt.Matern32(a, b, l=.05, sig=.6) + mt.ExpCovFun(a, b, l=.8)`` is a
``KernelSum`` of up to four structures, a nested model that the device evaluates as one kernel
(DESIGN.md section 24), and ``LocalRange`` wraps one of the four stationary kernels into a nonstationary
covariance with a local range at every location (``MRATree(..., local_range=lam)``, section 25).  Any
callable that produces none of these is treated as an opaque function and evaluated on the host block
by block.
"""
from __future__ import annotations

import numpy as np
from scipy.spatial.distance import cdist, pdist, squareform
from scipy.special import gamma, gammaln, kv

# kernel kinds understood by the HIP library (include/mra_hip.h: MRA_KERNEL_*)
KIND_EXP = 0
KIND_MATERN32 = 1
KIND_MATERN52 = 2
KIND_GAUSSIAN = 3
KIND_IDEN = 4
KIND_KANTER = 5
KIND_MATERN = 6            # Matern of any smoothness nu in [NU_MIN, NU_MAX]
KIND_SUM = 7               # a sum of up to SUM_MAX of the closed-form kinds below (KernelSum): a nested covariance model
KIND_LOCAL = 8             # local ranges in the last coordinate column (LocalRange): a nonstationary covariance
NU_MIN, NU_MAX = 0.1, 5.0
SUM_MAX = 4


class SymbolicLocs:
    """Stand-in for a location array while ``MRATree`` probes the ``cov`` callable."""
    __slots__ = ("tag", "ndim", "shape", "data")

    def __init__(self, tag, d, data=None):
        self.tag = tag
        self.ndim = 2
        self.shape = (0, d)
        self.data = data            # the caller's full location array (needed by KanterCovFun(radius=int))

    def __len__(self):
        return 1            # `if len(locs2)` in the reference's dist(): "second set given"


def _check_metric(A, circular=False):
    """The ``metric=`` argument of the kernels: None, or a square float64 matrix A (1 x 1 to 3 x 3; a scalar counts as 1 x 1) -
    distances are |A (a - b)|.  Its size against the locations is checked where both are known."""
    if A is None:
        return None
    A = np.array(A, dtype=np.float64)
    if A.ndim == 0:
        A = A.reshape(1, 1)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or not 1 <= A.shape[0] <= 3:
        raise ValueError("metric must be a d x d matrix with d = 1, 2 or 3, got shape %r" % (A.shape,))
    if circular:
        raise ValueError("metric= cannot be combined with circular=True: the torus has period 1 in the raw coordinate")
    return A


def _in_metric(locs, A):
    """locs @ A.T: the coordinates distances are taken on under metric=A (None for None or an empty second set)."""
    if A is None or locs is None or not len(locs):
        return locs
    locs = np.asarray(locs, dtype=np.float64)
    locs = locs if locs.ndim == 2 else locs.reshape(len(locs), 1)
    if locs.shape[1] != A.shape[0]:
        raise ValueError("metric is %d x %d but the locations have %d coordinates" % (A.shape[0], A.shape[0], locs.shape[1]))
    return locs @ A.T


class KernelSpec:
    """kind + (l, sig) + an overall scale; value = scale * k_kind(D; l, sig), D = |a - b| or, with a metric A, |A (a - b)|.
    nu: the smoothness of KIND_MATERN (None for every other kind)."""
    __slots__ = ("kind", "l", "sig", "scale", "circular", "A", "nu")

    def __init__(self, kind, l=1.0, sig=1.0, scale=1.0, circular=False, A=None, nu=None):
        self.kind, self.l, self.sig, self.scale, self.circular = int(kind), float(l), float(sig), float(scale), bool(circular)
        self.A = _check_metric(A, self.circular)
        self.nu = _check_nu(nu) if self.kind == KIND_MATERN else None

    def __mul__(self, c):
        if isinstance(c, (int, float, np.floating, np.integer)):
            return KernelSpec(self.kind, self.l, self.sig, self.scale * float(c), self.circular, self.A, self.nu)
        return NotImplemented

    __rmul__ = __mul__

    def __truediv__(self, c):
        return self.__mul__(1.0 / float(c))

    def __add__(self, other):
        """A nested model: the sum of two structures (or of a structure and a sum) is a KernelSum, evaluated on the device as one kernel."""
        if isinstance(other, (KernelSpec, KernelSum)):
            return KernelSum(_sum_parts(self) + _sum_parts(other))
        return NotImplemented

    def params(self):
        return np.array([self.l, self.sig, self.scale], dtype=np.float64)

    def evaluate(self, locs1, locs2):
        """Host evaluation (tests / diagnostics); same arithmetic as the array path below."""
        fn = _HOST_KERNELS[self.kind]
        locs1, locs2 = _in_metric(np.asarray(locs1), self.A), _in_metric(np.asarray(locs2), self.A)
        extra = (self.nu,) if self.kind == KIND_MATERN else ()
        return self.scale * np.asarray(fn(locs1, locs2, self.l, self.sig, self.circular, *extra))

    def __repr__(self):
        base = "KernelSpec(kind=%d, l=%g, sig=%g, scale=%g" % (self.kind, self.l, self.sig, self.scale)
        base += "" if self.nu is None else ", nu=%g" % self.nu
        return base + (")" if self.A is None else ", A=%s)" % np.array2string(self.A, separator=", ").replace("\n", ""))


_SUM_KINDS = (KIND_EXP, KIND_MATERN32, KIND_MATERN52, KIND_GAUSSIAN, KIND_IDEN)
_SUM_HAS_SIG = (KIND_MATERN32, KIND_MATERN52, KIND_GAUSSIAN)       # (ExpCovFun and Iden have no sig of their own: their sill is their scale)


def _sum_parts(k):
    """The components of a KernelSpec (itself) or of a KernelSum (each with the sum's scale folded into its own)."""
    if isinstance(k, KernelSum):
        return [c if k.scale == 1.0 else c * k.scale for c in k.components]
    return [k]


class KernelSum:
    """scale * (k_0 + ... + k_{K-1}), 1 <= K <= SUM_MAX components, each a KernelSpec of kind EXP, MATERN32, MATERN52, GAUSSIAN or IDEN
    with its own range, sill and scale; they share the distance: ``circular`` and the metric ``A`` are the sum's.  An Iden component
    is a micro-scale part of the field (its sill at D == 0, 0 elsewhere), not measurement noise.  kind = KIND_SUM, nu = None.

    ``l`` and ``sig`` are what ``HipPlan.set_kernel(kind, l, sig, scale, circular, nu)`` takes for kind 7, so that code written for a
    KernelSpec sends a sum unchanged: l = the components as (kind, l_c, sig_c) triples, sig_c the component's whole sill (its scale
    times its sig, for the kinds that have one); sig = the total sill at scale 1."""
    __slots__ = ("components", "scale", "circular", "A")
    kind = KIND_SUM
    nu = None

    def __init__(self, components, scale=1.0):
        comps = tuple(components)
        if not 1 <= len(comps) <= SUM_MAX:
            raise ValueError("a sum of kernels has 1 to %d components, got %d" % (SUM_MAX, len(comps)))
        for c in comps:
            if not isinstance(c, KernelSpec):
                raise TypeError("the components of a KernelSum are KernelSpecs, got %r" % (c,))
            if c.kind not in _SUM_KINDS:
                raise ValueError("a %s cannot be a component of a sum (ExpCovFun, Matern32, Matern52, GaussianCovFun and Iden can)"
                                 % ("Kanter taper" if c.kind == KIND_KANTER else "Matern(nu)" if c.kind == KIND_MATERN else "kernel of kind %d" % c.kind))
            if not (np.isfinite(c.l) and c.l > 0.0) or not (np.isfinite(c.scale * c.sig) and c.scale >= 0.0 and c.sig >= 0.0):
                raise ValueError("a component needs a positive range and a sill that is not negative, got %r" % (c,))
        first = comps[0]
        for c in comps[1:]:
            if c.circular != first.circular:
                raise ValueError("the components of a sum share one distance: all circular or none")
            if (c.A is None) != (first.A is None) or (c.A is not None and not np.array_equal(c.A, first.A)):
                raise ValueError("the components of a sum share one distance: their metrics differ")
        self.components, self.scale, self.circular, self.A = comps, float(scale), first.circular, first.A

    @property
    def l(self):
        return tuple((c.kind, c.l, c.scale * (c.sig if c.kind in _SUM_HAS_SIG else 1.0)) for c in self.components)

    @property
    def sig(self):
        return float(sum(t[2] for t in self.l))

    def __add__(self, other):
        if isinstance(other, (KernelSpec, KernelSum)):
            return KernelSum(_sum_parts(self) + _sum_parts(other))
        return NotImplemented

    def __mul__(self, c):
        if isinstance(c, (int, float, np.floating, np.integer)):
            return KernelSum(self.components, self.scale * float(c))
        return NotImplemented

    __rmul__ = __mul__

    def __truediv__(self, c):
        return self.__mul__(1.0 / float(c))

    def params(self):
        """The parameter vector of mra_plan_set_kernel(7, ...): {K, 0, scale, circular, kind_0, l_0, sig_0, ...}."""
        return np.array([len(self.components), 0.0, self.scale, 1.0 if self.circular else 0.0] + [v for t in self.l for v in t], dtype=np.float64)

    def evaluate(self, locs1, locs2):
        """Host evaluation: the NumPy sum of the components' own evaluations, in component order, times the sum's scale."""
        out = self.components[0].evaluate(locs1, locs2)
        for c in self.components[1:]:
            out = out + c.evaluate(locs1, locs2)
        return out if self.scale == 1.0 else self.scale * out

    def __repr__(self):
        return "KernelSum(%s%s)" % (" + ".join(repr(c) for c in self.components), "" if self.scale == 1.0 else ", scale=%g" % self.scale)


_LOCAL_BASES = (KIND_EXP, KIND_MATERN32, KIND_MATERN52, KIND_GAUSSIAN)      # scale mixtures of Gaussians: what the validity theorem needs


class LocalRange:
    """A nonstationary covariance with a local range lam(s) > 0 at every location (Paciorek & Schervish 2006, isotropic local kernels;
    DESIGN.md section 25).  The locations it is evaluated on carry their range in the LAST column: rows (x, lam) in 1-D, (x, y, lam) in
    2-D.  With ds spatial columns, D their Euclidean distance and q = (la^2 + lb^2) / 2,

        C(a, b) = scale * sig * (la lb / q)^(ds / 2) * k0(D / (l sqrt(q))),

    k0 the base kernel at range 1: ``base`` is a KernelSpec of kind EXP, MATERN32, MATERN52 or GAUSSIAN without circular distance or
    metric, whose l multiplies the whole range field.  A constant lam0 gives the stationary kernel of range l * lam0; C(a, a) is
    scale * sig.  kind = KIND_LOCAL, circular False, A and nu None.

    ``lam``: optionally the range field the spec was built for (MRATree keeps the tree's there); evaluate does not read it.
    ``l`` is what ``HipPlan.set_kernel(kind, l, sig, scale, circular)`` takes for kind 8, so that code written for a KernelSpec sends
    this one unchanged: the pair (base kind, l).  ``sig`` is the sill at scale 1 (1 for ExpCovFun, which has no sig)."""
    __slots__ = ("base", "lam")
    kind = KIND_LOCAL
    circular = False
    A = None
    nu = None

    def __init__(self, base, lam=None):
        if not isinstance(base, KernelSpec):
            raise TypeError("the base of a LocalRange is a KernelSpec, got %r" % (base,))
        if base.kind not in _LOCAL_BASES:
            raise ValueError("the base of a LocalRange must be ExpCovFun, Matern32, Matern52 or GaussianCovFun, got kind %d" % base.kind)
        if base.circular:
            raise ValueError("a LocalRange has no circular distance")
        if base.A is not None:
            raise ValueError("a LocalRange takes no metric: A would mix the range column into the distance")
        if not (np.isfinite(base.l) and base.l > 0.0 and np.isfinite(base.sig) and base.sig >= 0.0 and np.isfinite(base.scale)):
            raise ValueError("a LocalRange needs a positive l and a finite sill, got %r" % (base,))
        self.base = base
        self.lam = None if lam is None else _check_ranges(lam)

    @property
    def l(self):
        return (self.base.kind, self.base.l)

    @property
    def sig(self):
        return self.base.sig if self.base.kind != KIND_EXP else 1.0

    @property
    def scale(self):
        return self.base.scale

    def __mul__(self, c):
        if isinstance(c, (int, float, np.floating, np.integer)):
            return LocalRange(self.base * c, self.lam)
        return NotImplemented

    __rmul__ = __mul__

    def __truediv__(self, c):
        return self.__mul__(1.0 / float(c))

    def params(self):
        """The parameter vector of mra_plan_set_kernel(8, ...): {l, sig, scale, 0, base kind}."""
        return np.array([self.base.l, self.sig, self.scale, 0.0, self.base.kind], dtype=np.float64)

    def evaluate(self, locs1, locs2):
        """Host evaluation in float64 NumPy on arrays (n1, ds + 1) and (n2, ds + 1) whose last column is the range: the formula
        above, stated once - the oracles and the CPU twins use it as they use KernelSpec.evaluate."""
        a, b = np.asarray(locs1, dtype=np.float64), np.asarray(locs2, dtype=np.float64)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or a.shape[1] not in (2, 3):
            raise ValueError("a LocalRange is evaluated on (n, 2) rows (x, lam) or (n, 3) rows (x, y, lam)")
        ds = a.shape[1] - 1
        la, lb = a[:, -1][:, None], b[:, -1][None, :]
        if not (np.all(a[:, -1] > 0.0) and np.all(b[:, -1] > 0.0)):
            raise ValueError("the ranges (last column) must be positive")
        D2 = np.zeros((len(a), len(b)))
        for k in range(ds):
            D2 += np.square(a[:, k][:, None] - b[:, k][None, :])
        q = 0.5 * (la * la + lb * lb)
        u = (la * lb) / q
        pref = u if ds == 2 else np.sqrt(u)
        l, kind = self.base.l, self.base.kind
        if kind == KIND_GAUSSIAN:
            k0 = np.exp(-D2 / (2.0 * (l * l) * q))
        else:
            c = {KIND_EXP: 1.0, KIND_MATERN32: np.sqrt(3.0), KIND_MATERN52: np.sqrt(5.0)}[kind]
            t = c * np.sqrt(D2 / q) / l
            poly = 1.0 if kind == KIND_EXP else (1.0 + t if kind == KIND_MATERN32 else 1.0 + t + t * t / 3.0)
            k0 = poly * np.exp(-t)
        return (self.scale * self.sig) * (pref * k0)

    def __repr__(self):
        return "LocalRange(%r%s)" % (self.base, "" if self.lam is None else ", lam=<%d ranges>" % len(self.lam))


def _check_ranges(lam, n=None):
    """A range field: a 1-D array (of n values, when n is given) of finite positive numbers."""
    lam = np.asarray(lam, dtype=np.float64)
    if lam.ndim == 2 and lam.shape[1] == 1:
        lam = lam[:, 0]
    if lam.ndim != 1 or (n is not None and len(lam) != n):
        raise ValueError("local_range must be a 1-D array%s" % ("" if n is None else " of %d values" % n))
    if not (np.all(np.isfinite(lam)) and np.all(lam > 0.0)):
        raise ValueError("local ranges must be finite and positive")
    return np.ascontiguousarray(lam)


def _check_nu(nu):
    """The smoothness of KIND_MATERN: a finite number in [NU_MIN, NU_MAX], the range the device quadrature is accurate on."""
    if nu is None:
        raise ValueError("KIND_MATERN needs nu")
    nu = float(nu)
    if not (np.isfinite(nu) and NU_MIN <= nu <= NU_MAX):
        raise ValueError("nu must lie in [%g, %g], got %r" % (NU_MIN, NU_MAX, nu))
    return nu


def _symbolic(*args):
    return any(isinstance(a, SymbolicLocs) for a in args)


# ----------------------------------------------------------------------------------------
def genLocations(NGrid, lb=0, ub=1, random=False):
    if random:
        pts = np.random.uniform(lb, ub, NGrid)
    else:
        pts = np.linspace(lb, ub, num=NGrid + 1)[1:]
    return pts.reshape((NGrid, 1))


def genLocations2d(Nx, lbx=0, ubx=1, Ny=0, lby=0, uby=1):
    """Regular grid, x fastest: row i = (x[i mod Nx], y[i div Nx])."""
    if not Ny:
        Ny = Nx
    gx, gy = np.meshgrid(np.linspace(lbx, ubx, num=Nx), np.linspace(lby, uby, num=Ny))
    return np.hstack((gx.reshape(Nx * Ny, 1), gy.reshape(Nx * Ny, 1)))


# ---- points on a sphere: the covariance is evaluated on the chordal distance, the Euclidean distance of the points' 3-D
# coordinates (every stationary kernel here stays positive definite on it); the tree is still partitioned on (lon, lat)
def lonlat_to_xyz(lonlat, radius=1.0, degrees=True):
    """(n, 2) longitude / latitude -> (n, 3) Cartesian coordinates on the sphere of the given radius."""
    ll = np.asarray(lonlat, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[1] != 2:
        raise ValueError("lonlat must have shape (n, 2)")
    if degrees:
        ll = np.deg2rad(ll)
    lon, lat = ll[:, 0], ll[:, 1]
    cl = np.cos(lat)
    return float(radius) * np.column_stack((cl * np.cos(lon), cl * np.sin(lon), np.sin(lat)))


def chord_of_arc(theta, radius=1.0):
    """Chord length of a great-circle distance theta (a length on the sphere of the given radius): 2 R sin(theta / 2R).  States a
    range parameter given as a great-circle distance in the chordal metric the kernels are evaluated on."""
    return 2.0 * radius * np.sin(np.asarray(theta, dtype=np.float64) / (2.0 * radius))


def arc_of_chord(c, radius=1.0):
    """Great-circle distance of a chord length c: 2 R asin(c / 2R), the inverse of chord_of_arc."""
    return 2.0 * radius * np.arcsin(np.clip(np.asarray(c, dtype=np.float64) / (2.0 * radius), -1.0, 1.0))


def aniso2d(ratio, angle, degrees=True):
    """The 2 x 2 metric of geometric anisotropy: with a kernel of range l, the range is l along the major axis of correlation,
    which points along ``angle`` (counter-clockwise from the x axis), and l / ratio across it.  A = diag(1, ratio) R(-angle)."""
    ratio = float(ratio)
    if not ratio > 0.0:
        raise ValueError("ratio must be positive")
    th = np.deg2rad(float(angle)) if degrees else float(angle)
    c, s = np.cos(th), np.sin(th)
    return np.array([[c, s], [-ratio * s, ratio * c]])


def ard(lengths):
    """Per-axis ranges: diag(1 / lengths), to be used with l = 1 (space-time data on (x, y, t): ard([lx, ly, lt]))."""
    lengths = np.atleast_1d(np.asarray(lengths, dtype=np.float64))
    if lengths.ndim != 1 or not 1 <= len(lengths) <= 3 or not np.all(lengths > 0.0):
        raise ValueError("lengths must be 1 to 3 positive numbers")
    return np.diag(1.0 / lengths)


def dist(locs, locs2=np.array([]), circular=False):
    locs = locs if np.ndim(locs) == 2 else np.reshape(locs, [len(locs), 1])
    if circular:
        other = locs2 if len(locs2) else locs
        a, b = np.meshgrid(locs, other)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        return np.matrix(np.minimum(hi - lo, lo + 1 - hi).T)
    if len(locs2):
        locs2 = locs2 if np.ndim(locs2) == 2 else np.reshape(locs2, [len(locs2), 1])
        return np.matrix(cdist(locs, locs2))
    return np.matrix(squareform(pdist(locs)))


def _exp(l1, l2, l, sig, circular):
    return np.exp(-dist(l1, l2, circular) / l)


def _m32(l1, l2, l, sig, circular):
    D = dist(l1, l2, circular)
    return sig * np.multiply(1 + np.sqrt(3) * D / l, np.exp(-np.sqrt(3) * D / l))


def _m52(l1, l2, l, sig, circular):
    D = dist(l1, l2, circular)
    return sig * np.multiply(1 + np.sqrt(5) * D / l + (5 / 3) * np.square(D / l), np.exp(-np.sqrt(5) * D / l))


def _gauss(l1, l2, l, sig, circular):
    D = dist(l1, l2, circular)
    return sig * np.exp(-np.square(D) / (2 * (l ** 2)))


def _iden(l1, l2, l, sig, circular):
    D = dist(l1, l2, circular)
    out = np.matrix(np.zeros(D.shape))
    out[np.where(D == 0)] = 1
    return out


def _kanter(l1, l2, l, sig, circular):
    """Kanter's compactly supported taper with radius l (pyMRA/MRATools.py:318-323)."""
    D = np.array(dist(l1, l2, circular)) / l
    with np.errstate(divide="ignore", invalid="ignore"):
        p2 = 2 * np.pi * D
        R = (1 - D) * np.sin(p2) / p2 + 1 / np.pi * (1 - np.cos(p2)) / p2
    R[D > 1] = 0
    R[D == 0] = 1
    return R


def _matern_quad(t, nu, h=0.1):
    """t^nu K_nu(t) for 2^-5 <= t < 2 by the trapezoid rule on K_nu(t) = int_0^inf exp(-t cosh u) cosh(nu u) du - the device's method
     at half its step, all terms positive - by octaves of t, each with the nodes its smallest t needs."""
    out = np.empty_like(t)
    e = np.floor(np.log2(t))
    for ex in np.unique(e):
        idx = np.flatnonzero(e == ex)
        n = int(np.arccosh(745.0 / 2.0 ** ex) / h) + 2
        u = h * np.arange(n)
        w = h * np.cosh(nu * u)
        w[0] *= 0.5
        for i0 in range(0, len(idx), 1 << 16):          # (the len x n matrix of terms, 64 MB at a time)
            ts = t[idx[i0:i0 + (1 << 16)]]
            out[idx[i0:i0 + (1 << 16)]] = ts ** nu * np.sum(w * np.exp(-np.outer(ts, np.cosh(u))), axis=1)
    return out


def matern_nu(t, nu):
    """M_nu(t) = 2^(1-nu) / Gamma(nu) t^nu K_nu(t) for t >= 0, M_nu(0) = 1, to 1e-15 against 40-digit values.  scipy.special.kv, but on
    2^-5 <= t < 2 - where kv's power series loses a digit for fractional nu (1.5e-14 at nu = 0.8, t = 1.9) - the quadrature of
    _matern_quad; 0 at t > 700 (M_nu < 1e-290, t^nu K_nu underflows); the leading terms 1 - Gamma(1-nu) / Gamma(1+nu) (t/2)^(2 nu) at
    t < 2^-40 (what is left out is below 1e-21)."""
    t = np.asarray(t, dtype=np.float64)
    out = np.ones_like(t)
    big, tiny = t > 700.0, (t > 0.0) & (t < 2.0 ** -40)
    low = (t >= 2.0 ** -5) & (t < 2.0)
    mid = (t >= 2.0 ** -40) & ~low & ~big
    c = 2.0 ** (1.0 - nu) / gamma(nu)
    out[mid] = c * (t[mid] ** nu * kv(nu, t[mid]))
    out[low] = c * _matern_quad(t[low], nu)
    out[big] = 0.0
    if nu < 1.0:
        out[tiny] = 1.0 - np.exp(gammaln(1.0 - nu) - gammaln(1.0 + nu) + 2.0 * nu * np.log(0.5 * t[tiny]))
    return out


def _matern(l1, l2, l, sig, circular, nu=1.5):
    D = np.asarray(dist(l1, l2, circular))
    return sig * matern_nu(np.sqrt(2.0 * nu) * D / l, nu)


_HOST_KERNELS = {KIND_EXP: _exp, KIND_MATERN32: _m32, KIND_MATERN52: _m52, KIND_GAUSSIAN: _gauss,
                 KIND_IDEN: _iden, KIND_KANTER: _kanter, KIND_MATERN: _matern}


def determine_radius(k, h, ndim=2):
    """Taper radius that leaves about k grid points inside the support (mesh width h); same rule as
    pyMRA/MRATools.py:329-388: 1 grid row -> int(k/2) h; otherwise the ring of the square lattice whose
    cumulative point count is nearest to k."""
    if ndim == 1:
        return int(k / 2) * h
    if k == 0:
        raise ValueError("Ensemble size must be stricly positive")
    s = np.floor(np.sqrt(k))
    sf = s - 1 if s % 2 == 0 else s
    if k == sf ** 2:
        return h * 1.01 * (sf - 1) / 2 * np.sqrt(2)
    base = (sf - 1) / 2.0
    counts = [sf ** 2]
    while counts[-1] < (sf + 2) ** 2:
        step = 4 if (len(counts) == 1 or (sf + 2) ** 2 - counts[-1] == 4) else 8
        counts.append(counts[-1] + step)
    counts = np.asarray(counts)
    ind = counts.searchsorted(k)
    pick = ind - 1 if k <= (counts[ind - 1] + counts[ind]) / 2.0 else ind
    if pick == 0:
        return h * base * np.sqrt(2) + h * 0.01
    return h * np.sqrt((base + 1) ** 2 + (pick - 1) ** 2) + h * 0.01


def KanterCovFun(locs, locs2=np.array([]), radius=1.0, circular=False, metric=None):
    """radius: float = taper radius; int = target number of points in the support (resolved from the grid
    spacing of ``locs`` like the reference does; on the device path from the tree's full location set)."""
    src = locs.data if isinstance(locs, SymbolicLocs) else locs
    if isinstance(radius, int):
        if src is None:
            raise ValueError("KanterCovFun(radius=int) needs the locations to derive the mesh width")
        xs = np.sort(np.unique(src[:, 0]))
        ndim = len(np.unique(src[:, 1])) if src.shape[1] > 1 else 1
        radius = determine_radius(radius, xs[1] - xs[0], ndim=ndim)
    metric = _check_metric(metric, circular)
    if _symbolic(locs, locs2):
        return KernelSpec(KIND_KANTER, radius, 1.0, 1.0, circular, metric)
    return _kanter(_in_metric(locs, metric), _in_metric(locs2, metric), radius, 1.0, circular)


def Iden(locs, locs2=np.array([]), l=1, circular=False, metric=None):
    metric = _check_metric(metric, circular)
    if _symbolic(locs, locs2):
        return KernelSpec(KIND_IDEN, l, 1.0, 1.0, circular, metric)
    return _iden(_in_metric(locs, metric), _in_metric(locs2, metric), l, 1.0, circular)


def ExpCovFun(locs, locs2=np.array([]), l=1, circular=False, metric=None):
    metric = _check_metric(metric, circular)
    if _symbolic(locs, locs2):
        return KernelSpec(KIND_EXP, l, 1.0, 1.0, circular, metric)
    return _exp(_in_metric(locs, metric), _in_metric(locs2, metric), l, 1.0, circular)


def Matern52(locs, locs2=np.array([]), l=1, sig=1, circular=False, metric=None):
    metric = _check_metric(metric, circular)
    if _symbolic(locs, locs2):
        return KernelSpec(KIND_MATERN52, l, sig, 1.0, circular, metric)
    return np.matrix(_m52(_in_metric(locs, metric), _in_metric(locs2, metric), l, sig, circular))


def Matern32(locs, locs2=np.array([]), l=1, sig=1, circular=False, metric=None):
    metric = _check_metric(metric, circular)
    if _symbolic(locs, locs2):
        return KernelSpec(KIND_MATERN32, l, sig, 1.0, circular, metric)
    return np.matrix(_m32(_in_metric(locs, metric), _in_metric(locs2, metric), l, sig, circular))


def GaussianCovFun(locs, locs2=np.array([]), l=1, sig=1, circular=False, metric=None):
    metric = _check_metric(metric, circular)
    if _symbolic(locs, locs2):
        return KernelSpec(KIND_GAUSSIAN, l, sig, 1.0, circular, metric)
    return np.matrix(_gauss(_in_metric(locs, metric), _in_metric(locs2, metric), l, sig, circular))


def Matern(locs, locs2=np.array([]), l=1, sig=1, nu=1.5, circular=False, metric=None):
    """Matern covariance of any smoothness 0.1 <= nu <= 5: sig * 2^(1-nu) / Gamma(nu) * t^nu * K_nu(t), t = sqrt(2 nu) D / l (sklearn's
    parametrisation, which Matern32 and Matern52 share).  The reference's Matern(locs, l, sig, nu) has no ``locs2`` and cannot serve as
    a tree's ``cov``; this one has the shape of its siblings and can.  With the symbolic locations of a tree it returns the kernel's
    spec - nu of exactly 0.5, 1.5 or 2.5 the closed forms (KIND_EXP with scale sig, KIND_MATERN32, KIND_MATERN52: the same functions
    on faster kernels), any other nu KIND_MATERN, evaluated on the device by quadrature; with arrays it evaluates on the host (``matern_nu``):
    scipy.special.kv, except on 2^-5 <= t < 2, where kv misses 5e-15 for fractional nu and the trapezoid sum for K_nu - the integral
    representation the device uses, at half its step - takes over.  On that range, where most covariance values of a tree lie, the
    oracles and CPU twins built on this function therefore share the device's method; what keeps the two independent there is the
    40-digit mpmath table (tests/golden/matern_nu.npz), which both are tested against."""
    metric = _check_metric(metric, circular)
    nu = _check_nu(nu)
    if _symbolic(locs, locs2):
        if nu == 0.5:
            return KernelSpec(KIND_EXP, l, 1.0, float(sig), circular, metric)
        if nu == 1.5 or nu == 2.5:
            return KernelSpec(KIND_MATERN32 if nu == 1.5 else KIND_MATERN52, l, sig, 1.0, circular, metric)
        return KernelSpec(KIND_MATERN, l, sig, 1.0, circular, metric, nu)
    return np.matrix(_matern(_in_metric(locs, metric), _in_metric(locs2, metric), l, sig, circular, nu))
