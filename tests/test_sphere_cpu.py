"""Covariances on 3-D coordinates, the host side: the lon/lat helpers of MRATools, the ``coord_dim`` field of
the topology (the tree never depends on it) and the host-evaluated blocks on xyz.  No GPU."""
import dataclasses

import numpy as np
import pytest

import _cases as K  # noqa: F401  (puts the repository on sys.path)
import pymra_amd.MRATools as mt
from pymra_amd.plan import host_cov_blocks
from pymra_amd.sharding import shard_topology
from pymra_amd.topology import build_topology


def _grid(nx, ny):
    lon = -180.0 + (np.arange(nx) + 0.5) * 360.0 / nx
    lat = np.linspace(-80.0, 80.0, ny)
    g, h = np.meshgrid(lon, lat)
    return np.column_stack((g.ravel(), h.ravel()))


def test_lonlat_to_xyz_is_on_the_sphere_and_round_trips():
    rng = np.random.default_rng(1)
    ll = np.column_stack((rng.uniform(-180, 180, 500), rng.uniform(-90, 90, 500)))
    for radius in (1.0, 6371.0):
        x = mt.lonlat_to_xyz(ll, radius)
        assert x.shape == (500, 3)
        assert np.max(np.abs(np.linalg.norm(x, axis=1) - radius)) <= 4e-16 * radius
        lon = np.degrees(np.arctan2(x[:, 1], x[:, 0]))
        lat = np.degrees(np.arcsin(x[:, 2] / radius))
        assert np.max(np.abs(lon - ll[:, 0])) < 1e-11 and np.max(np.abs(lat - ll[:, 1])) < 1e-11
    rad = mt.lonlat_to_xyz(np.radians(ll), degrees=False)
    assert np.max(np.abs(rad - mt.lonlat_to_xyz(ll))) < 1e-15
    with pytest.raises(ValueError):
        mt.lonlat_to_xyz(np.zeros((4, 3)))


def test_chords_and_arcs():
    for radius in (1.0, 2.5):
        a = mt.lonlat_to_xyz(np.array([[10.0, 20.0], [-170.0, -20.0]]), radius)          # antipodes
        assert abs(np.linalg.norm(a[0] - a[1]) - 2.0 * radius) < 1e-15 * radius
        assert abs(mt.arc_of_chord(2.0 * radius, radius) - np.pi * radius) < 1e-15
        theta = np.linspace(0.0, np.pi * radius, 50)
        assert np.max(np.abs(mt.arc_of_chord(mt.chord_of_arc(theta, radius), radius) - theta)) < 2e-8 * radius       # asin near 1
        assert np.max(np.abs(mt.arc_of_chord(mt.chord_of_arc(theta[:40], radius), radius) - theta[:40])) < 1e-14 * radius
    # across the date line: lon +179.9 and -179.9 on the equator are 0.2 degrees apart
    b = mt.lonlat_to_xyz(np.array([[179.9, 0.0], [-179.9, 0.0]]))
    arc = mt.arc_of_chord(np.linalg.norm(b[0] - b[1]))
    assert abs(np.degrees(arc) - 0.2) < 1e-12
    assert abs(mt.chord_of_arc(np.radians(0.2)) - np.linalg.norm(b[0] - b[1])) < 1e-16


def test_coord_dim_does_not_touch_the_tree():
    ll = _grid(48, 24)
    np.random.seed(3)
    plain = build_topology(ll, 16, 2, 4)
    np.random.seed(3)
    sph = build_topology(ll, 16, 2, 4, coord_dim=3)
    assert plain.coord_dim == 0 and sph.coord_dim == 3 and sph.d == 2
    for f in dataclasses.fields(plain):
        if f.name in ("coord_dim", "node_ident"):
            continue
        a, b = getattr(plain, f.name), getattr(sph, f.name)
        assert np.array_equal(np.asarray(a), np.asarray(b)), f.name
    assert list(plain.node_ident) == list(sph.node_ident)
    for native in (True, False):                      # the Python replay carries the field as the native one does
        np.random.seed(3)
        assert build_topology(ll, 16, 2, 4, native=native, coord_dim=3).coord_dim == 3
    for world in (2, 4):
        for rank in range(world):
            lt, _ = shard_topology(sph, world, rank)
            assert lt.coord_dim == 3 and lt.d == 2
    with pytest.raises(ValueError):
        build_topology(ll, 16, 2, 4, coord_dim=4)


def test_host_cov_blocks_see_the_covariance_coordinates():
    ll = _grid(32, 16)
    xyz = mt.lonlat_to_xyz(ll)
    np.random.seed(5)
    topo = build_topology(ll, 16, 1, 4, coord_dim=3)
    rng = np.random.default_rng(2)
    y = np.where(rng.random(len(ll)) < 0.4, rng.standard_normal(len(ll)), np.nan)
    spec = mt.KernelSpec(mt.KIND_MATERN32, 0.5)
    seen = []

    def cov(a, b):
        seen.append((np.shape(a)[1], np.shape(b)[1]))
        return spec.evaluate(a, b)

    S = np.asarray(spec.evaluate(xyz, xyz))
    n = 0
    for (i, C, dg), (i2, C2, dg2) in zip(host_cov_blocks(topo, cov, xyz, y), host_cov_blocks(topo, S, xyz, y)):
        assert i == i2 and C.shape == C2.shape
        assert np.max(np.abs(C - C2)) < 1e-15 if C.size else True
        assert (dg is None) == (dg2 is None)
        if dg is not None:
            assert np.max(np.abs(dg - dg2)) < 1e-15
        n += 1
    assert n == topo.n_nodes and set(seen) == {(3, 3)}
