"""The decision rule of fps_prefix_kernel (csrc/fps.hip, prcnn_fps_nested), restated and held to the oracle on the CPU.

A nested FPS level samples the cloud S' = gather(S, prev_idx) the parent level produced.  The kernel answers a frame with
positions 0, 1, 2, ... when every coordinate of S' satisfies fabsf(c) < 1e4f and prev_idx[j] != 0 for 1 <= j < npoint.  Here:
under the canonical tie order the rule never accepts a longer prefix than prcnn_cpu_fps_mode confirms, level by level, on
eight cloud families (plain, degenerate, non-finite); on the plain ones it accepts everything (so the test cannot pass
vacuously); and under the upstream tie order a lattice breaks the prefix property itself, which is why that order takes no hint.
"""
import numpy as np
import pytest

N0 = 2048
LEVELS = (512, 128, 32)          # 2048 -> 512 -> 128 -> 32


def _uniform(rng):
    return rng.uniform([-40, -3, 0], [40, 1, 70], (N0, 3))


def _lattice(rng):
    g = np.stack(np.meshgrid(np.arange(16), np.arange(8), np.arange(16), indexing="ij"), -1).reshape(-1, 3) * 0.5
    return g[rng.permutation(len(g))]


def _distinct100(rng):
    return rng.uniform(-10, 10, (100, 3))[rng.integers(0, 100, N0)]


def _wrapped37(rng):
    return rng.uniform(-10, 10, (37, 3))[np.arange(N0) % 37]           # the RoI clouds' wrap padding


def _quantised(rng):
    return np.round(rng.uniform(0, 3, (N0, 3)) * 4) / 4


def _identical(rng):
    return np.tile(rng.uniform(-10, 10, (1, 3)), (N0, 1))


def _one_nan(rng):
    p = _uniform(rng)
    p[777, 1] = np.nan
    return p


def _one_huge(rng):
    p = _uniform(rng)
    p[1300, 2] = 3e30
    return p


FAMILIES = {"uniform": _uniform, "lattice": _lattice, "distinct100": _distinct100, "wrapped37": _wrapped37, "quantised": _quantised,
            "identical": _identical, "one_nan": _one_nan, "one_huge": _one_huge}
PLAIN = ("uniform", "lattice")


def rule_prefix(xyz, prev_idx, npoint):
    """the prefix length fps_prefix_kernel's two tests vouch for; the kernel accepts the frame iff this equals npoint"""
    with np.errstate(invalid="ignore"):
        if not bool(np.all(np.abs(xyz.astype(np.float32)) < np.float32(1e4))):          # NaN, inf: the comparison is false
            return 0
    again = np.nonzero(prev_idx[1:npoint] == 0)[0]
    return int(again[0]) + 1 if len(again) else npoint


def true_prefix(idx):
    """leading positions j with idx[j] == j"""
    miss = np.nonzero(idx != np.arange(len(idx)))[0]
    return int(miss[0]) if len(miss) else len(idx)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_rule_never_accepts_more_than_the_oracle_confirms(cpu, family):
    rng = np.random.default_rng(sorted(FAMILIES).index(family) + 11)
    cloud = FAMILIES[family](rng).astype(np.float32)[None]
    prev = cpu.fps_mode(cloud, LEVELS[0])
    for npoint in LEVELS[1:]:
        cloud = np.take_along_axis(cloud, prev[:, :, None].astype(np.int64), axis=1)
        want = cpu.fps_mode(cloud, npoint)
        assert np.array_equal(want, cpu.fps(cloud, npoint))
        accepted, true = rule_prefix(cloud[0], prev[0], npoint), true_prefix(want[0])
        assert accepted <= true, (family, cloud.shape[1], npoint, accepted, true)
        if accepted == npoint:          # what the kernel then writes
            assert np.array_equal(want[0], np.arange(npoint))
        if family in PLAIN:
            assert accepted == npoint, (family, cloud.shape[1], npoint, accepted)
        if family in ("one_nan", "one_huge"):
            assert accepted == 0            # the bad point is the parent's second sample, so it is in every nested cloud
        prev = want


def test_upstream_order_breaks_the_prefix_property_on_a_lattice(cpu):
    """argmin (k mod T, k) among equal maxima is not "lowest position": on a lattice (ties at every step) the upstream-order FPS of a
    sample set in sample order is NOT 0, 1, 2, ... -- while the canonical order on the same cloud is.  order="upstream" takes no hint.
    (The two orders are the same rule when N is a power of two up to 1 024, where T = N: the nested cloud here has 1 536 points.)"""
    cloud = _lattice(np.random.default_rng(5)).astype(np.float32)[None]
    for order in (0, 1):
        prev = cpu.fps_mode(cloud, 1536, order=order)
        nested = np.take_along_axis(cloud, prev[:, :, None].astype(np.int64), axis=1)
        got = cpu.fps_mode(nested, 384, order=order)
        if order == 0:
            assert true_prefix(got[0]) == 384
        else:
            assert np.array_equal(got, cpu.fps_upstream(nested, 384))
            assert true_prefix(got[0]) == 82            # (recorded from the oracle; DESIGN 4.1 quotes it)
