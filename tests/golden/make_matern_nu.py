"""Writes tests/golden/matern_nu.npz: M_nu(t) = 2^(1-nu) / Gamma(nu) t^nu K_nu(t) from mpmath at 40 digits, rounded to float64.

    nu      the ten smoothnesses of the tests
    t       t = 0, 25 points 2^-40 ... 2^-4 (exponents in steps of 1.5), 180 points 0.1 ... 45 (equally spaced)
    M       (len(nu), len(t)) values, M[:, 0] = 1
    t_edge  2^-60, 2^-41 (below the quadrature's clamp), 100, 700 (the far tail)
    M_edge  (len(nu), len(t_edge))

Run from the repository root:  python tests/golden/make_matern_nu.py
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 40
NU = [0.1, 0.25, 0.5, 0.8, 1.0, 1.5, 2.0, 2.5, 3.3, 5.0]


def matern(nu, t):
    if t == 0:
        return mp.mpf(1)
    nu, t = mp.mpf(nu), mp.mpf(t)
    return mp.power(2, 1 - nu) / mp.gamma(nu) * mp.power(t, nu) * mp.besselk(nu, t)


def main():
    t = np.concatenate(([0.0], 2.0 ** np.linspace(-40.0, -4.0, 25), np.linspace(0.1, 45.0, 180)))
    t_edge = np.array([2.0 ** -60, 2.0 ** -41, 100.0, 700.0])
    M = np.array([[float(matern(nu, x)) for x in t] for nu in NU])
    M_edge = np.array([[float(matern(nu, x)) for x in t_edge] for nu in NU])
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "matern_nu.npz")
    np.savez_compressed(out, nu=np.array(NU), t=t, M=M, t_edge=t_edge, M_edge=M_edge)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
