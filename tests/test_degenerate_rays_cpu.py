"""CPU half of the degenerate-ray tests: the inputs of tests/test_degenerate_rays_gpu.py through the oracle alone, and the table limits.

The oracle (the reference's extension / shadow stages in binary32 with denormals) must itself be well behaved on rays with NaN, infinite,
signed-zero, denormal, huge or tiny components: it returns, it never reports a NaN distance, the classes that can hit do hit (a
condition on the INPUTS: a census of misses only would make the GPU comparison empty), and the classes include/gmupt.h calls a miss are
the miss record.  The closest-hit tmax rule of include/gmupt.h has no oracle stage of its own (an extension ray has no limit): its
expected records are derived from the FLT_MAX records by trace_util.expected_closest_with_tmax, which is checked here against the
sentence it restates.
"""
import numpy as np
import pytest

import trace_util as T


@pytest.fixture(scope="module")
def soup(pkg):
    return pkg.scenes.build_scene(pkg.scenes.random_triangles_mesh(2000, seed=1))


def test_the_oracle_defines_every_class(pkg, oracle, soup):
    n = 1024
    lc = soup["light_count"]
    census = {}
    for name, (closest, any_rays) in T.degenerate_classes(soup, n).items():
        truth = T.oracle_truth(soup, closest, any_rays, lc)                       # returns: every walk ends
        assert not np.isnan(truth["hitDistance"][:n, 0].view(np.float32)).any(), name
        hits, occ = int((truth["triangle"][:n, 0] != T.NO_TRI).sum()), int(truth["inShadow"][:n, 0].sum())
        census[name] = (hits, occ)
        print("%-18s %4d triangle hits, %4d occluded of %d" % (name, hits, occ, n))
        if name in T.MISS_CLASSES:
            assert T.is_miss_record(truth, n).all() and not truth["isEmitter"][:n, 0].any(), (name, hits, occ)
    # floors on the inputs (the oracle alone): 100 of 1024
    for name in ("denormal_inf", "denormal_finite", "denormal_two", "negzero_component", "signed_zero_axis", "huge_direction"):
        assert census[name][0] >= 100, (name, census[name])
    for name in ("denormal_inf", "denormal_finite", "denormal_two", "negzero_component", "signed_zero_axis"):
        assert census[name][1] >= 100, (name, census[name])
    # any-hit tmax: 0, -1 and NaN never occlude (a length is never below them); +inf and FLT_MAX are no limit; 1e-45 is below every length here
    closest, any_rays = T.degenerate_classes(soup, n)["tmax_any"]
    occ = T.oracle_truth(soup, closest, any_rays, lc)["inShadow"][:n, 0]
    tmax = any_rays[:, 3]
    with np.errstate(invalid="ignore"):
        assert not occ[~(tmax > 0)].any() and (~(tmax > 0)).sum() >= n // 2 - 1
    unlimited = any_rays.copy(); unlimited[:, 3] = np.inf
    occ_inf = T.oracle_truth(soup, closest, unlimited, lc)["inShadow"][:n, 0]
    assert occ_inf.sum() >= 100 and np.array_equal(occ[np.isposinf(tmax)], occ_inf[np.isposinf(tmax)])
    assert np.array_equal(occ[tmax == T.FLT_MAX], occ_inf[tmax == T.FLT_MAX])


def test_the_mixed_batches_hold_what_they_promise(pkg, oracle, soup):
    # k lanes of every 64-ray wave are degenerate, the others are the ordinary rays untouched (bitwise), and those have normal non-zero components
    for k in (1, 7, 32, 63):
        closest, any_rays, mask, base_c, base_a = T.mixed_rays(soup, 4096, k, seed=5)
        assert (mask.reshape(-1, 64).sum(axis=1) == k).all()
        assert np.array_equal(closest[~mask].view(np.uint32), base_c[~mask].view(np.uint32)) and np.array_equal(any_rays[~mask].view(np.uint32), base_a[~mask].view(np.uint32))
        d = base_c[:, 4:7]
        assert (np.abs(d) >= T.FLT_MIN).all() and np.isfinite(np.float32(1.0) / d).all()
        with np.errstate(all="ignore"):
            special = ~np.isfinite(np.float32(1.0) / closest[:, 4:7]).all(axis=1)       # the rays that send a wave to the general slab test
        assert special[mask].sum() >= (k * 64) // 4 and not special[~mask].any()
    truth = T.oracle_truth(soup, closest, any_rays, soup["light_count"])
    assert not np.isnan(truth["hitDistance"][:4096, 0].view(np.float32)).any()


def test_closest_tmax_rule_of_the_header(pkg, oracle, soup):
    # include/gmupt.h: tmax <= 0 (-0.0 included) or NaN: the miss record with t = the bits of tmax; +inf: the FLT_MAX record, a miss has t = +inf
    n = 1024
    closest, _ = T.random_rays(soup, n, np.random.default_rng(5))
    truth = T.oracle_truth(soup, closest, closest[:0], 0)
    rec = np.zeros((n, 8), np.uint32)
    hit = truth["triangle"][:n, 0] != T.NO_TRI
    rec[:, 0] = truth["hitDistance"][:n, 0]; rec[:, 1:3] = np.where(hit[:, None], truth["baryCoord"][:n, 1:3], 0)
    rec[:, 3] = np.where(hit, 7, T.NO_TRI)
    tmax = T.CLOSEST_TMAX[np.arange(n) % len(T.CLOSEST_TMAX)]
    exp = T.expected_closest_with_tmax(rec, tmax)
    inf = np.isposinf(tmax)
    assert (hit & inf).sum() >= 50 and (~hit & inf).sum() >= 50
    assert np.array_equal(exp[inf & hit], rec[inf & hit])
    assert (exp[inf & ~hit, 0].view(np.float32) == np.inf).all() and np.array_equal(exp[inf & ~hit, 1:], rec[inf & ~hit, 1:])
    assert np.array_equal(exp[~inf, 0], tmax.view(np.uint32)[~inf]) and (exp[~inf, 3] == T.NO_TRI).all() and not exp[~inf][:, [1, 2, 4, 5, 6, 7]].any()
    assert {int(b) for b in exp[~inf, 0]} == {0x00000000, 0x80000000, 0xBF800000, 0x7FC00000}


def test_wide_table_limits(pkg):
    # the wide ray cast's signed 32-bit byte offsets: 128-byte nodes, 48-byte references plus their sentinel, 80-byte pairs, each below 2^31
    fits = pkg.capi.wide_tables_addressable
    nodes, tris, pairs = (1 << 31) // 128, -(-(1 << 31) // 48) - 1, -(-(1 << 31) // 80)      # the first count of each table that does not fit
    assert nodes * 128 >= 1 << 31 > (nodes - 1) * 128 and (tris + 1) * 48 >= 1 << 31 > tris * 48 and pairs * 80 >= 1 << 31 > (pairs - 1) * 80
    assert fits(0, 0, 0) and fits(nodes - 1, tris - 1, pairs - 1)
    assert not fits(nodes, 0, 0) and fits(nodes - 1, 0, 0)
    assert not fits(0, tris, 0) and fits(0, tris - 1, 0)
    assert not fits(0, 0, pairs) and fits(0, 0, pairs - 1)
    assert not fits(nodes, tris - 1, pairs - 1) and not fits(nodes - 1, tris, pairs - 1) and not fits(nodes - 1, tris - 1, pairs)
    top = (1 << 32) - 1
    assert not fits(top, 0, 0) and not fits(0, top, 0) and not fits(0, 0, top)       # (numTris + 1 must not wrap)
