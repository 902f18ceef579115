"""MRA_OPT_PARENT_PAIR (GPU only): the fronts of the leaves' parents in four-wave workgroups, two to a CU (k_parent_front_pair<17|23>)
instead of one eight-wave workgroup per CU (k_parent_front).  Which wave owns a tile changes nothing in the tile's arithmetic - the
same k order, the same panel factorisation, the same Schur expression - so every result must be BITWISE what option 0 gives, and
option 0 is the kernel that the parity tests pin to the oracle.

Two regular trees, one plan each, the option switched 0 -> 2 -> 0 -> 2 (2: the pair kernel wherever the fronts fit, whatever the
number of CUs):
    (128, 32, 5)  1024 leaves, fronts of 66 tiles  -> k_parent_front_pair<17>
    (256, 32, 6)  4096 leaves, fronts of 91 tiles  -> k_parent_front_pair<23>
Under a 40 % mask a leaf has one or two 16-column steps of observations, a front 0 to 8 K steps: the shortest loops, where a mistake
in the step table, the first request or the reuse of the stages for the panel shows.  Forced on top: a family of four empty leaves
(no K step at all: the front is the identity), a family with one non-empty child, a leaf of exactly 16 and one of exactly 17
observations, four families of three and four of two children; fronts with an odd and with an even number of steps in the same launch.

That the pair kernel ran is read from the executed-flop count of its family: its empty accumulator slots (two of 68, one of 92)
run a tile once more per K step, which the plan accounts as executed - not algorithmic - work."""
import numpy as np
import pytest

import test_gpu_likelihood_masks as MK

pytestmark = pytest.mark.gpu

OPT = 23                                   # MRA_OPT_PARENT_PAIR
VISITS = (0, 2, 0, 2)
TREES = {(128, 32, 5): dict(leaves=1024, tiles=66, nacc=17), (256, 32, 6): dict(leaves=4096, tiles=91, nacc=23)}
FAMILY = "k_parent_front"
EMPTY_FAMILY, ONE_CHILD_FAMILY, FIRST_EXACT_FAMILY = 2, 5, 8
THREE_CHILD_FAMILIES, TWO_CHILD_FAMILIES = (40, 41, 42, 43), (44, 45, 46, 47)
TAGS = ("predict", "likelihood", "predict again")


@pytest.fixture(scope="module")
def hip(built_library):
    from pymra_amd import plan
    if plan.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    assert plan.MRA_OPT_PARENT_PAIR == OPT
    return plan


def build_case(tree):
    """Topology, locations, mask and the leaves forced to exact counts: {leaf position: count}."""
    topo, locs = MK._tree(*tree)
    rng = np.random.RandomState(0)
    obs = rng.uniform(size=topo.N) < 0.4
    fams = MK._families(topo)
    pos = {i: p for p, i in enumerate(int(i) for i in np.nonzero(topo.node_leaf)[0])}
    exact = {}
    MK._empty(obs, topo, fams[EMPTY_FAMILY])
    exact.update({pos[i]: 0 for i in fams[EMPTY_FAMILY]})
    f = fams[ONE_CHILD_FAMILY]
    MK._empty(obs, topo, f[:-1])
    MK._exact(obs, topo, f[-1], 5, rng)
    exact.update({pos[i]: 0 for i in f[:-1]})
    exact[pos[f[-1]]] = 5
    want = [16, 17]                        # each in the first leaf of at least 17 rows of a family of its own
    k = FIRST_EXACT_FAMILY
    while want:
        big = [i for i in fams[k] if len(MK._leaf_callers(topo, i)) >= 17]
        if big:
            c = want.pop(0)
            MK._exact(obs, topo, big[0], c, rng)
            exact[pos[big[0]]] = c
        k += 1
    for k in THREE_CHILD_FAMILIES:         # fronts of three and of two children: step counts of either parity beside the usual four
        MK._empty(obs, topo, fams[k][:1])
    for k in TWO_CHILD_FAMILIES:
        MK._empty(obs, topo, fams[k][1:3])
    return dict(topo=topo, locs=locs, obs=obs, exact=exact, y=MK._y(obs), counts=MK.leaf_counts(topo, obs))


@pytest.fixture(scope="module", params=sorted(TREES), ids=lambda t: "%dx%d_r%d_M%d" % (t[0], t[0], t[1], t[2]))
def case(request):
    c = build_case(request.param)
    c["tree"] = request.param
    return c


def front_steps(counts):
    """K steps of every parent front: its four children's observation tiles."""
    return ((np.asarray(counts) + 15) // 16).reshape(-1, 4).sum(axis=1)


def test_the_mask_has_every_kind_of_front(case):
    counts, want = case["counts"], TREES[case["tree"]]
    assert len(counts) == want["leaves"] and all(counts[p] == c for p, c in case["exact"].items())
    assert sorted(case["exact"].values()) == [0] * 7 + [5, 16, 17]
    tiles = (counts + 15) // 16
    assert int(tiles.max()) == 2 and (tiles == 1).sum() > 100 and (tiles == 2).sum() >= 2
    steps = front_steps(counts)
    print("fronts by K steps:", np.bincount(steps).tolist())
    assert steps[EMPTY_FAMILY] == 0 and steps[ONE_CHILD_FAMILY] == 1            # the identity alone; one child, one step
    assert all(steps[k] in (3, 4) for k in THREE_CHILD_FAMILIES) and all(steps[k] in (2, 3) for k in TWO_CHILD_FAMILIES)
    assert (steps % 2 == 1).sum() >= 5 and (steps % 2 == 0).sum() >= 5          # odd and even step counts in one launch
    assert 2 <= int(np.median(steps)) and int(steps.max()) <= 8


def _passes(pl):
    """A likelihood + predict pass, a likelihood-only pass, a second predict pass; the parent-front family's record of each."""
    out = {}
    for tag, predict in zip(TAGS, (True, False, True)):
        pl.run(True, predict)
        fam = [k for k in pl.kernel_stats() if k["name"].startswith(FAMILY)]
        assert len(fam) == 1, [k["name"] for k in pl.kernel_stats()]
        out[tag] = dict(lik=pl.likelihood(), route=pl.route(), launches=fam[0]["launches"], flops=fam[0]["flops"], flops_exec=fam[0]["flops_exec"])
        if predict:
            m, v = pl.predict()
            out[tag].update(mean=m.copy(), var=v.copy())
    return out


@pytest.fixture(scope="module")
def runs(hip, case):
    """[results of visit k] on ONE plan."""
    s = MK._spec()
    pl = hip.HipPlan(case["topo"], 0)
    pl.set_locs(case["locs"]); pl.set_obs(case["y"], MK.R); pl.set_kernel(s.kind, s.l, s.sig, s.scale)
    assert pl.get_option(OPT) == 1
    out = []
    for v in VISITS:
        pl.set_option(OPT, v)
        assert pl.get_option(OPT) == v
        out.append(_passes(pl))
    pl.close()
    return out


def _same(a, b, what):
    for tag in TAGS:
        assert a[tag]["lik"] == b[tag]["lik"], (what, tag, a[tag]["lik"], b[tag]["lik"])
        assert a[tag]["route"] == b[tag]["route"], (what, tag)
        if "mean" in a[tag]:
            assert np.array_equal(a[tag]["mean"], b[tag]["mean"]), (what, tag, "mean")
            assert np.array_equal(a[tag]["var"], b[tag]["var"]), (what, tag, "var")


def test_the_results_are_finite_and_the_fronts_went_through_one_launch(runs):
    for k, res in enumerate(runs):
        for tag in TAGS:
            r = res[tag]
            assert np.isfinite(r["lik"]).all(), (k, tag)
            assert r["route"]["path"] == "Fused" and r["route"]["parent_front"], (k, tag, r["route"])
            assert r["launches"] == 1, (k, tag, r["launches"])
            if "mean" in r:
                assert np.isfinite(r["mean"]).all() and (r["var"] >= 0).all() and (r["var"] > 0).any(), (k, tag)


def test_the_pair_kernel_ran_under_setting_two_only(case, runs):
    """Its empty slots' executed flops, exactly: (4 NACC - tiles) slots x K steps of all fronts x four 16 x 16 x 4 MFMAs."""
    want = TREES[case["tree"]]
    idle = float(front_steps(case["counts"]).sum()) * (4 * want["nacc"] - want["tiles"]) * 4 * (2 * 16 * 16 * 4)
    assert idle > 0
    for tag in TAGS:
        assert runs[0][tag]["flops_exec"] == runs[2][tag]["flops_exec"] and runs[1][tag]["flops_exec"] == runs[3][tag]["flops_exec"]
        assert abs(runs[1][tag]["flops_exec"] - runs[0][tag]["flops_exec"] - idle) <= 1e-6 * idle, (tag, runs[1][tag]["flops_exec"], runs[0][tag]["flops_exec"], idle)
        assert runs[1][tag]["flops"] == runs[0][tag]["flops"], tag


def test_passes_are_bitwise_those_of_the_eight_wave_kernel(runs):
    _same(runs[0], runs[1], "setting 2 against 0")
    for res in runs:
        assert res["predict"]["lik"] == res["predict again"]["lik"]
        assert np.array_equal(res["predict"]["mean"], res["predict again"]["mean"]) and np.array_equal(res["predict"]["var"], res["predict again"]["var"])
        assert sum(res["likelihood"]["lik"]) == pytest.approx(sum(res["predict"]["lik"]), rel=1e-12)


def test_a_second_visit_reproduces_the_first(runs):
    _same(runs[0], runs[2], "setting 0, second visit")
    _same(runs[1], runs[3], "setting 2, second visit")
