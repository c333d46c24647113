"""Seeded two-view scenes for the monocular Initializer: K = TUM1, float32 pixel coordinates.

Every scene has N matches of which a share are outliers (wrong partner at least 20 px away),
inlier noise of at most 0.3 px, unmatched keys on both sides (so Normalize sees more keys than
matches), -1 holes in matches12 and n2 != n1.
"""
import numpy as np

K = np.array([[517.3, 0.0, 318.6], [0.0, 516.5, 255.3], [0.0, 0.0, 1.0]], np.float32)
KINDS = ("general", "planar", "rotation", "low_parallax", "few_good")


def _rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def scene(kind, seed, N, outliers=0.0, extra=(7, 4), noise=0.3, tiny=False, plane=None, motion=None):
    """-> dict(K, keys1 (n1 x 2), keys2 (n2 x 2), matches12 (n1), R, t, X (n1 x 3, NaN where not a
    true correspondence), genuine (n1 bool))."""
    assert kind in KINDS
    rng = np.random.default_rng([seed, KINDS.index(kind), N])
    Kd = K.astype(np.float64)
    R = _rodrigues([0.02, -0.05, 0.015])
    t = np.array([-0.45, 0.03, 0.02])
    u1 = np.stack([rng.uniform(30, 610, N), rng.uniform(30, 450, N)], axis=1)
    z = rng.uniform(3.0, 8.0, N)
    if kind == "planar":
        # the plane n . X = d through the view: depth from the pixel ray
        n, d = (np.array([0.9, -0.3, 1.0]), 5.0) if plane is None else plane
        t = np.array([-1.5, 0.0, 0.0]) if motion is None else np.asarray(motion, np.float64)
        rays = np.concatenate([u1, np.ones((N, 1))], axis=1) @ np.linalg.inv(Kd).T
        z = d / (rays @ n)
    elif kind == "rotation":
        R, t = _rodrigues([0.03, -0.08, 0.02]), np.zeros(3)
    elif kind == "low_parallax":
        t = np.array([-0.04, 0.002, 0.001]) * (0.2 if tiny else 1.0)
        z = rng.uniform(2.0, 12.0, N)
    rays = np.concatenate([u1, np.ones((N, 1))], axis=1) @ np.linalg.inv(Kd).T
    X = rays * z[:, None]
    x2 = (X @ R.T + t) @ Kd.T
    u2 = x2[:, :2] / x2[:, 2:3]
    u1n = u1 + rng.uniform(-noise, noise, (N, 2))
    u2n = u2 + rng.uniform(-noise, noise, (N, 2))
    genuine = np.ones(N, bool)
    n_out = int(round(outliers * N))
    if kind == "few_good":
        n_out = max(n_out, N - 45)
    bad = rng.permutation(N)[:n_out]
    for i in bad:
        while True:
            p = np.array([rng.uniform(10, 630), rng.uniform(10, 470)])
            if np.linalg.norm(p - u2[i]) >= 20:
                break
        u2n[i] = p
        genuine[i] = False
    e1, e2 = extra
    n1, n2 = N + e1, N + e2
    slot1, slot2 = rng.permutation(n1), rng.permutation(n2)
    keys1 = np.stack([rng.uniform(10, 630, n1), rng.uniform(10, 470, n1)], axis=1)
    keys2 = np.stack([rng.uniform(10, 630, n2), rng.uniform(10, 470, n2)], axis=1)
    keys1[slot1[:N]], keys2[slot2[:N]] = u1n, u2n
    m12 = np.full(n1, -1, np.int32)
    m12[slot1[:N]] = slot2[:N]
    Xk = np.full((n1, 3), np.nan)
    Xk[slot1[:N]] = np.where(genuine[:, None], X, np.nan)
    gk = np.zeros(n1, bool)
    gk[slot1[:N]] = genuine
    return dict(K=K.copy(), keys1=keys1.astype(np.float32), keys2=keys2.astype(np.float32), matches12=m12,
                R=R, t=t, X=Xk, genuine=gk, kind=kind, N=N)
