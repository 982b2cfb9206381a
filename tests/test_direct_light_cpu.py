"""The slot-class preconditions of test_direct_light_gpu.py on the CPU oracle alone: every set-up of direct_light_util.py holds the slots it
is run for, so the GPU tests cannot pass vacuously.  Needs no device."""
import numpy as np
import pytest

import direct_light_util as D
import oracle_lib as O
import shade_util as S


@pytest.fixture(scope="module")
def scene(pkg):
    return S.edge_scene(pkg)


def _oracle_keeps_the_sentinels(c):
    dl = O.state_field(c.orc.path_state(), D.P, "directLight")
    kept = np.ones(D.P, bool); kept[:D.L] = c.kind != "S"
    assert np.array_equal(dl[kept], c.sent[kept])
    assert ((dl != c.sent).any(axis=1) == ~kept).all() and int((~kept).sum()) == int(c.orc.counters()[6])


def test_sentinels_are_distinct_and_hold_nans():
    s = D.sentinels(D.P)
    assert len(np.unique(s)) == s.size
    nan = D._is_nan(s)
    assert nan[1::4].all() and nan[3::4].all() and not nan[0::2].any()


def test_midflight_pool_holds_every_kind(pkg, scene):
    c = D.Crafted(pkg, scene, S.block_layout(2), path_budget=D.L + D.MIDFLIGHT_REFILL, max_depth=D.MIDFLIGHT_DEPTH)
    for k in "ESNGR":
        assert (c.kind == k).any(), "no slot of kind %s in the pool" % k
    assert 0 < c.orc.active_paths() < D.L
    _oracle_keeps_the_sentinels(c)
    c.close()


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_block_layout_preconditions(pkg, scene, variant):
    c = D.Crafted(pkg, scene, S.block_layout(variant))
    D.layout_preconditions(c.kind, variant)
    _oracle_keeps_the_sentinels(c)
    c.close()


@pytest.mark.parametrize("light_count", [1, D.MAX_LIGHTS])
def test_operand_preconditions(pkg, light_count):
    c = D.Crafted(pkg, D.operand_scene(pkg), D.operand_layout(), light_count=light_count, far=True)
    D.operand_preconditions(c, light_count)
    _oracle_keeps_the_sentinels(c)
    c.close()
