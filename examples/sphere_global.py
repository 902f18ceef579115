#!/usr/bin/env python3
"""Global data on a sphere: a Matern-3/2 field on a lon/lat grid with a swath-shaped gap that crosses the date line.  The tree is
partitioned on (lon, lat) as for any 2-D data; the covariance is evaluated on the chordal distance (metric="chordal": the kernels see
the points' xyz), so lon -180 and +180 are the same meridian and the poles are points.  Fit, predict on a finer grid that fills the
gap, and draw the field there once.

    python examples/sphere_global.py [n_lon] [n_lat] [M] [r0]
"""
import sys

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pymra_amd.MRATools as mt
from pymra_amd import MRATree


def lonlat_grid(n_lon, n_lat, lat_max=85.0):
    lon = -180.0 + (np.arange(n_lon) + 0.5) * 360.0 / n_lon
    g, h = np.meshgrid(lon, np.linspace(-lat_max, lat_max, n_lat))
    return np.column_stack((g.ravel(), h.ravel()))


def main():
    n_lon = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    n_lat = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    M = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    r0 = int(sys.argv[4]) if len(sys.argv) > 4 else 32
    np.random.seed(31)
    ll = lonlat_grid(n_lon, n_lat)
    # the range as a great-circle distance (2000 km on an Earth of radius 6371 km), stated in the chordal metric of the unit sphere
    l = float(mt.chord_of_arc(2000.0 / 6371.0))
    cov = lambda a, b: mt.Matern32(a, b, l=l, sig=1.0)
    R = 0.02
    blank = np.full((len(ll), 1), np.nan)
    blank[0] = 0.0                                    # the tree needs one observed row; a prior draw ignores it
    truth = MRATree(ll, r0, cov, blank, R, M=M, J=4, metric="chordal").simulate(1, "prior", seed=3)[:, 0]
    # a swath 30 degrees wide, tilted against the meridians, centred on the date line: not observed
    d_lon = (ll[:, 0] - 0.4 * ll[:, 1]) % 360.0 - 180.0               # signed distance in longitude from the centre line lon = 180 + 0.4 lat
    gap = np.abs(d_lon) < 15.0
    y = np.where(gap, np.nan, truth + np.sqrt(R) * np.random.normal(size=len(ll))).reshape(-1, 1)
    tree = MRATree(ll, r0, cov, y, R, M=M, J=4, metric="chordal")
    print("%d x %d lon/lat grid, %d observed, %d in the gap across the date line; likelihood %.3f"
          % (n_lon, n_lat, int(np.isfinite(y).sum()), int(gap.sum()), float(tree.getLikelihood()[0, 0])))
    mean, sd = tree.predict()
    err = np.asarray(mean).ravel() - truth
    print("rmse at observed rows %.3f, inside the gap %.3f (predictive sd there %.3f)"
          % (np.sqrt(np.mean(err[~gap] ** 2)), np.sqrt(np.mean(err[gap] ** 2)), float(np.mean(sd[gap]))))

    fine = lonlat_grid(2 * n_lon, 2 * n_lat)          # sites are (lon, lat) in degrees as well
    m, s = tree.predictAt(fine)
    # (the date line is also a boundary of the lon/lat partition: inside the unobserved swath the two sides are predicted from their
    # own leaves and the shared coarse levels only, so the mean has the jump an MRA has at any partition boundary - it shrinks with
    # r0 and M; the kernel itself sees the two sides as the 1.4 degrees apart they are)
    west, east = fine[:, 0] < -179.0, fine[:, 0] > 179.0
    print("finer grid %d x %d: mean in [%.3f, %.3f]; inside the gap the two sides of the date line differ by %.4f on average (sd there %.3f)"
          % (2 * n_lon, 2 * n_lat, m.min(), m.max(), float(np.abs(m[west, 0] - m[east, 0]).mean()), float(s[west | east].mean())))
    draw = tree.sampleAt(fine, 1, "posterior", seed=5)[:, 0]
    print("one posterior draw on the finer grid: in [%.3f, %.3f], rms distance from the mean %.3f" % (draw.min(), draw.max(), np.sqrt(np.mean((draw - m[:, 0]) ** 2))))


if __name__ == "__main__":
    main()
