"""Shared by the tests of the pose stage (gmupt_pose_host, gmupt_pose_*): an independent numpy restatement of the rule of include/gmupt.h
("Pose"), binary32 throughout, written from the header's text, and the random rigs the tests run it on.

Every statement is one elementwise float32 operation on whole arrays (a product, then a sum: numpy rounds each to binary32 and never
contracts), in the header's order: targets ascending, influences ascending, the bracketing of q as written.  Skipped terms are skipped by
np.where on the weight, so that an infinity or a NaN behind a zero weight never enters an operation whose result is kept."""
import numpy as np


def rule(rest, joints, weights, num_joints, joint_mats, deltas=None, target_weights=None):
    """The posed vertices of the rule as a (V, 3) float32 array."""
    R = np.ascontiguousarray(rest, np.float32).reshape(-1, 3)
    V, J = R.shape[0], int(num_joints)
    D = np.zeros((0, V, 3), np.float32) if deltas is None else np.ascontiguousarray(deltas, np.float32).reshape(-1, V, 3)
    T = D.shape[0]
    a = np.zeros(T, np.float32) if target_weights is None else np.ascontiguousarray(target_weights, np.float32).reshape(-1)
    assert J or T
    with np.errstate(all="ignore"):
        m = [R[:, c].copy() for c in range(3)]
        for t in range(T):                                        # 1. morph
            if a[t] != np.float32(0.0):
                for c in range(3):
                    prod = a[t] * D[t, :, c]
                    m[c] = m[c] + prod
                    assert m[c].dtype == np.float32
        if not J:
            return np.stack(m, axis=1)
        W = np.ascontiguousarray(weights, np.float32).reshape(V, -1)
        K = W.shape[1]
        jn = np.ascontiguousarray(joints, np.uint16).reshape(V, K).astype(np.int64)
        M = np.ascontiguousarray(joint_mats, np.float32).reshape(J, 3, 4)
        p = [np.zeros(V, np.float32) for _ in range(3)]
        any_ = np.zeros(V, bool)
        for k in range(K):                                        # 2. skin
            w = W[:, k]
            on = w != np.float32(0.0)
            j = np.where(on, jn[:, k], 0)                         # the joint number of a zero weight is never followed
            assert np.all(j < J), "rule 4"
            for c in range(3):
                t0 = M[j, c, 0] * m[0]
                t1 = M[j, c, 1] * m[1]
                s = t0 + t1
                t2 = M[j, c, 2] * m[2]
                s = s + t2
                q = s + M[j, c, 3]
                wq = w * q
                acc = p[c] + wq
                assert acc.dtype == np.float32
                p[c] = np.where(on, acc, p[c])
            any_ |= on
        return np.stack([np.where(any_, p[c], m[c]) for c in range(3)], axis=1).astype(np.float32)   # 3. result


def random_rig(V, K, J, T, seed):
    """A random rig and pose: rest in [-4, 4), weights positive with about a quarter of them exactly zero (either sign) and the joint
    number of such an influence anything at all, matrices near the identity, deltas small, one target weight zero when T > 1."""
    rng = np.random.default_rng([V, K, J, T, seed])
    rig = {"rest": rng.uniform(-4, 4, (V, 3)).astype(np.float32), "num_joints": J, "joints": None, "weights": None, "mats": None}
    rig["rest"][rig["rest"] == 0] = 1.0
    if J:
        w = rng.uniform(0.05, 1.0, (V, K)).astype(np.float32)
        j = rng.integers(0, J, (V, K)).astype(np.uint16)
        off = rng.random((V, K)) < 0.25
        w[off] = np.where(rng.random(int(off.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
        j[off] = rng.integers(0, 65536, int(off.sum())).astype(np.uint16)
        rig["weights"], rig["joints"] = w, j
        mats = np.tile(np.eye(3, 4, dtype=np.float32).reshape(12), (J, 1)) + rng.normal(0, 0.2, (J, 12)).astype(np.float32)
        rig["mats"] = mats.astype(np.float32)
    rig["deltas"] = rng.normal(0, 0.3, (T, V, 3)).astype(np.float32)
    tw = rng.uniform(-1, 1, T).astype(np.float32)
    tw[tw == 0] = 0.5
    if T > 1:
        tw[int(rng.integers(0, T))] = 0.0
    rig["target_weights"] = tw
    return rig


def host(capi, rig, threads=16, mats=None, target_weights=None):
    return capi.pose_host(rig["rest"], rig["joints"], rig["weights"], rig["num_joints"], rig["mats"] if mats is None else mats,
                          rig["deltas"], rig["target_weights"] if target_weights is None else target_weights, threads=threads)


def restated(rig, mats=None, target_weights=None):
    return rule(rig["rest"], rig["joints"], rig["weights"], rig["num_joints"], rig["mats"] if mats is None else mats,
                rig["deltas"], rig["target_weights"] if target_weights is None else target_weights)


def differing(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1, 3), np.ascontiguousarray(b, np.float32).reshape(-1, 3)
    return int(np.any(a.view(np.uint32) != b.view(np.uint32), axis=1).sum())
