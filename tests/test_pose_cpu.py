"""gmupt_pose_host, the reference of the device pose stage (include/gmupt.h "Pose"), against the independent numpy restatement of the rule
in pose_util.py -- bit for bit -- plus the rule's corner cases, the argument errors, the synthetic rig of scenes.py and its file format.
No device."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import pose_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gmupt_pose_host", "gmupt_pose_create", "gmupt_pose_update", "gmupt_pose_update_device", "gmupt_pose_destroy"]
CASES = list(itertools.product((1, 65, 1000), (1, 4, 8), (1, 3, 40), (0, 1, 3)))      # num_verts, K, J, T

IDENTITY = np.eye(3, 4, dtype=np.float32).reshape(12)
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def test_host_rule_equals_the_restatement_bit_for_bit(pkg):
    assert len(CASES) == 81
    for V, K, J, T in CASES:
        rig = PU.random_rig(V, K, J, T, 0)
        got = PU.host(pkg.capi, rig)
        assert got.shape == (V, 3) and got.dtype == np.float32
        n = PU.differing(got, PU.restated(rig))
        assert n == 0, "V %d K %d J %d T %d: %d vertices differ from the restatement" % (V, K, J, T, n)
    # enough vertices for several bands of the host's 4096-vertex chunks
    rig = PU.random_rig(3 * 4096 + 17, 4, 40, 3, 1)
    assert PU.differing(PU.host(pkg.capi, rig), PU.restated(rig)) == 0


def test_thread_counts_give_the_same_bytes(pkg):
    for V, K, J, T in [(1, 4, 3, 1), (65, 8, 40, 3), (1000, 4, 40, 3), (3 * 4096 + 17, 4, 40, 3)]:
        rig = PU.random_rig(V, K, J, T, 2)
        one = PU.host(pkg.capi, rig, threads=1).tobytes()
        for threads in (3, 16):
            assert PU.host(pkg.capi, rig, threads=threads).tobytes() == one, (V, threads)


def test_zero_target_weights_are_skipped_not_multiplied(pkg):
    rig = PU.random_rig(65, 4, 3, 3, 3)
    for zero in (np.float32(0.0), np.float32(-0.0)):
        for poison in (INF, -INF, NAN):
            tw = rig["target_weights"].copy(); tw[:] = (0.7, zero, -0.3)
            clean = dict(rig, deltas=rig["deltas"].copy()); clean["deltas"][1] = 0.0
            dirty = dict(rig, deltas=rig["deltas"].copy()); dirty["deltas"][1] = poison
            want = PU.host(pkg.capi, clean, target_weights=tw)
            got = PU.host(pkg.capi, dirty, target_weights=tw)
            assert np.all(np.isfinite(got)) and got.tobytes() == want.tobytes(), (zero, poison)
            assert PU.differing(got, PU.restated(dirty, target_weights=tw)) == 0
    # the control: with a weight that is not zero the poison arrives
    tw = np.array([0.7, 1e-30, -0.3], np.float32)
    dirty = dict(rig, deltas=rig["deltas"].copy()); dirty["deltas"][1] = INF
    assert not np.any(np.isfinite(PU.host(pkg.capi, dirty, target_weights=tw)[np.any(rig["weights"] != 0, axis=1)]))


def test_zero_influences_are_skipped_not_multiplied(pkg):
    V, K, J = 65, 4, 3
    rig = PU.random_rig(V, K, J, 1, 4)
    rig["weights"][:] = np.abs(rig["weights"]) + np.float32(0.1)
    rig["joints"][:] = np.arange(V * K).reshape(V, K) % 2                         # joints 0 and 1 carry the weights
    for zero in (np.float32(0.0), np.float32(-0.0)):
        w = rig["weights"].copy(); j = rig["joints"].copy()
        w[:, 2] = zero; j[:, 2] = 2                                             # joint 2 only behind zero weights
        for poison in (INF, NAN):
            mats = rig["mats"].copy(); mats[2, 4:8] = poison                    # a matrix row of inf / NaN
            got = pkg.capi.pose_host(rig["rest"], j, w, J, mats, rig["deltas"], rig["target_weights"])
            assert np.all(np.isfinite(got)), (zero, poison)
            assert got.tobytes() == pkg.capi.pose_host(rig["rest"], j, w, J, rig["mats"], rig["deltas"], rig["target_weights"]).tobytes()
            assert PU.differing(got, PU.rule(rig["rest"], j, w, J, mats, rig["deltas"], rig["target_weights"])) == 0
        j[:, 2] = 65535                                                         # any joint number behind a zero weight
        assert pkg.capi.pose_host(rig["rest"], j, w, J, rig["mats"], rig["deltas"], rig["target_weights"]).tobytes() == got.tobytes()


def test_a_vertex_without_influences_follows_the_morph_only(pkg):
    rig = PU.random_rig(65, 4, 3, 3, 5)
    rig["joints"][:] %= 3
    rig["weights"][::3] = 0.0
    rig["weights"][1::3][rig["weights"][1::3] == 0] = 0.5
    got = PU.host(pkg.capi, rig)
    morph = pkg.capi.pose_host(rig["rest"], None, None, 0, None, rig["deltas"], rig["target_weights"])
    assert got[::3].tobytes() == morph[::3].tobytes()
    assert PU.differing(got[1::3], morph[1::3]) == len(got[1::3])
    assert PU.differing(got, PU.restated(rig)) == 0


def test_morph_only_and_skin_only(pkg):
    rig = PU.random_rig(1000, 4, 40, 3, 6)
    morph = pkg.capi.pose_host(rig["rest"], None, None, 0, None, rig["deltas"], rig["target_weights"])
    assert PU.differing(morph, PU.rule(rig["rest"], None, None, 0, None, rig["deltas"], rig["target_weights"])) == 0
    assert PU.differing(morph, rig["rest"]) == 1000
    skin = pkg.capi.pose_host(rig["rest"], rig["joints"], rig["weights"], 40, rig["mats"])
    assert PU.differing(skin, PU.rule(rig["rest"], rig["joints"], rig["weights"], 40, rig["mats"])) == 0
    # target weights that are all zero are no targets
    assert skin.tobytes() == pkg.capi.pose_host(rig["rest"], rig["joints"], rig["weights"], 40, rig["mats"], rig["deltas"], np.zeros(3, np.float32)).tobytes()


def test_identity_matrices_return_the_rest_pose(pkg):
    rig = PU.random_rig(1000, 2, 3, 2, 7)
    assert not np.any(np.signbit(rig["rest"]) & (rig["rest"] == 0))             # the rule turns -0 into +0; the fixture has none
    rig["weights"][:] = 0.5
    rig["joints"][:] = [0, 2]
    mats = np.tile(IDENTITY, (3, 1))
    got = pkg.capi.pose_host(rig["rest"], rig["joints"], rig["weights"], 3, mats, rig["deltas"], np.zeros(2, np.float32))
    assert np.array_equal(got, rig["rest"])
    # and the sign the header speaks of
    rest = rig["rest"].copy(); rest[0, 0] = -0.0
    got = pkg.capi.pose_host(rest, rig["joints"], rig["weights"], 3, mats)
    assert got[0, 0] == 0 and not np.signbit(got[0, 0])


def test_argument_errors_write_nothing(pkg):
    capi = pkg.capi
    lib = capi.lib()
    V, K, J, T = 20, 4, 3, 2
    rig = PU.random_rig(V, K, J, T, 8)
    rig["weights"][rig["weights"] == 0] = 0.25
    rig["joints"][:] %= J
    out = np.full((V, 3), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    r, j, w, m, d, a = (rig[k] for k in ("rest", "joints", "weights", "mats", "deltas", "target_weights"))
    bad = j.copy(); bad[9, 1] = J
    good = (p(r), V, p(j), p(w), K, p(m), J, p(d), p(a), T, p(out))
    assert lib.gmupt_pose_host(*good, 4) == 0 and not np.any(out == 7.0)
    out[:] = 7.0

    def with_(**kw):
        names = ["rest", "V", "joints", "weights", "K", "mats", "J", "deltas", "tw", "T", "out"]
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return args

    calls = [with_(rest=None), with_(out=None), with_(V=0), with_(joints=None), with_(weights=None), with_(mats=None), with_(deltas=None),
             with_(tw=None), with_(K=0), with_(K=9), with_(J=65536), with_(T=257), with_(J=0, T=0), with_(joints=p(bad))]
    for args in calls:
        assert lib.gmupt_pose_host(*args, 4) == capi.ERR_INVALID_ARGUMENT, args
        assert np.all(out == 7.0)
    assert b"gmupt_pose_host" in lib.gmupt_last_error()
    with pytest.raises(capi.GmuptError) as e:
        capi.pose_host(r, bad, w, J, m, d, a)
    assert e.value.code == capi.ERR_INVALID_ARGUMENT
    # the same joint number on a weight of zero is no error
    w0 = w.copy(); w0[9, 1] = 0.0
    assert capi.pose_host(r, bad, w0, J, m, d, a).shape == (V, 3)


def test_make_rig_is_deterministic_and_normalised(pkg):
    S = pkg.scenes
    mesh = S.cornell_mesh()
    a, b = S.make_rig(mesh, 4, 4, 2, seed=3), S.make_rig(mesh, 4, 4, 2, seed=3)
    for k in ("rest", "joints", "weights", "deltas"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["deltas"].tobytes() != S.make_rig(mesh, 4, 4, 2, seed=4)["deltas"].tobytes()
    V = len(mesh["verts"])
    assert a["rest"].tobytes() == np.ascontiguousarray(mesh["verts"], np.float32).tobytes()
    assert a["joints"].shape == (V, 4) and a["joints"].dtype == np.uint16 and a["weights"].dtype == np.float32 and a["deltas"].shape == (2, V, 3)
    assert int(a["joints"].max()) < 4 and np.all(a["weights"] > 0)
    assert np.abs(a["weights"].sum(axis=1, dtype=np.float64) - 1.0).max() < 4 * 2.0 ** -23          # four float32 roundings of a sum near 1
    # more influences than joints: the spare ones carry no weight
    c = S.make_rig(mesh, 2, 4, 0, seed=0)
    assert np.all(c["weights"][:, 2:] == 0) and np.all(c["weights"][:, :2] > 0) and c["deltas"].shape == (0, V, 3)
    # rig_pose: phase 0 is the rest pose, another phase is not; both deterministic
    m0, t0 = S.rig_pose(a, 0.0)
    assert m0.shape == (4, 12) and m0.dtype == np.float32 and t0.shape == (2,) and np.all(t0 == 0)
    assert np.array_equal(m0, np.tile(IDENTITY, (4, 1)))
    m1, t1 = S.rig_pose(a, 0.3)
    assert m1.tobytes() == S.rig_pose(a, 0.3)[0].tobytes() and np.all(t1 != 0)
    posed = pkg.capi.pose_host(a["rest"], a["joints"], a["weights"], 4, m1, a["deltas"], t1)
    assert np.all(np.isfinite(posed)) and PU.differing(posed, a["rest"]) > V // 2
    assert np.abs(posed - a["rest"]).max() < 0.5 * a["extent"]
    morph_only = S.make_rig(mesh, 0, 0, 2, seed=3)
    assert morph_only["joints"] is None and S.rig_pose(morph_only, 0.3)[0].shape == (0, 12)


def test_grig_round_trip(pkg, tmp_path):
    S = pkg.scenes
    mesh = S.cornell_mesh()
    for J, K, T in ((4, 4, 2), (0, 0, 2), (3, 8, 0)):
        rig = S.make_rig(mesh, J, K, T, seed=1)
        path = str(tmp_path / ("rig_%d_%d_%d.grig" % (J, K, T)))
        S.save_grig(rig, path)
        V = len(mesh["verts"])
        assert os.path.getsize(path) == 24 + 12 * V + (6 * K * V if J else 0) + 12 * T * V
        back = S.load_grig(path)
        assert back["num_joints"] == J and back["deltas"].shape == (T, V, 3)
        for k in ("rest", "joints", "weights", "deltas"):
            if rig[k] is None:
                assert back[k] is None, k
            else:
                assert back[k].dtype == rig[k].dtype and back[k].tobytes() == rig[k].tobytes(), k
    with open(path, "ab") as f:
        f.write(b"\0")
    with pytest.raises(ValueError):
        S.load_grig(path)


def test_new_symbols_are_declared_bound_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "gmupt.h")).read()
    declared = set(re.findall(r"\b(gmupt_\w+)\(", header))
    lib = pkg.capi.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in pkg.capi.SYMBOLS, name
        assert getattr(lib, name, None) is not None, name
    assert C.sizeof(pkg.capi.PoseInfo) == 16
    assert hasattr(pkg.progressive.ProgressiveSession, "set_pose")
