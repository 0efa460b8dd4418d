"""NumPy restatement of the robust registration of ``csrc/teaser.hip`` (the TEASER++ depth refiner) for its tests, and the
seeded inputs those tests share.  Float64 by default; ``dtype=np.float32`` runs the same formulae in float32 (the tests take the
difference of the two runs as the scale of legitimate round-off).

The definition, per prediction, M <= 1024 correspondences ``b ~ R a + t``, ``beta = 2 noise_bound sqrt(cbar2)``,
``alpha = noise_bound sqrt(cbar2)``:
  graph        i ~ j (i != j) when | |b_j - b_i| - |a_j - a_i| | < beta
  clique       greedy: C = all; repeat: v = argmax popcount(adj[v] & C) over v in C (ties: lowest index), append, C &= adj[v];
               fewer than 3 members: rejected (-2)
  rotation     chain measurements between consecutive clique members (sorted by index); GNC-TLS with nb^2 = beta^2, w = 1,
               R from the SVD of sum w a b^T, mu = 1 / (2 max r^2 / nb^2 - 1) on the first iteration (<= 0: stop), TLS weight
               update, cost = sum w r^2 with the weights that produced R, stop on |cost - cost_prev| < 1e-12 or 100 iterations,
               mu <- 1.4 mu
  translation  per axis truncated least squares over the clique's members: candidates = midpoints of consecutive sorted
               interval ends x_i -+ alpha, cost = sum_S (x_i - mean_S)^2 / alpha^2 + (m - |S|) cbar2, lowest candidate of a tie
  accept       #{i: |R a_i + t - b_i| < noise_bound} >= min_num_inliers over all M, else rejected (-3)
"""

import numpy as np

MAX_POINTS = 1024


def fps(points, k, dtype=np.float64):
    """Farthest-point sampling: ``min(k, N)`` indices in selection order.  Starts at index 0; each step takes the point whose
    (squared) distance to the chosen set is largest, a tie goes to the lowest index."""
    P = np.asarray(points, dtype)
    N = len(P)
    M = min(k, N)
    idx = np.zeros(M, np.int64)
    if M == 0:
        return idx
    mind = np.full(N, np.inf, dtype)
    for s in range(1, M):
        d = P - P[idx[s - 1]]
        mind = np.minimum(mind, d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        idx[s] = int(np.argmax(mind))  # argmax: the first of equal maxima
    return idx


def pair_gaps(a, b, dtype=np.float64):
    """``| |b_j - b_i| - |a_j - a_i| |`` for every pair, [M, M]."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    da = a[None] - a[:, None]
    db = b[None] - b[:, None]
    na = np.sqrt(da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1] + da[..., 2] * da[..., 2])
    nb = np.sqrt(db[..., 0] * db[..., 0] + db[..., 1] * db[..., 1] + db[..., 2] * db[..., 2])
    return np.abs(nb - na)


def consistency_graph(a, b, noise_bound=0.01, cbar2=1.0, dtype=np.float64):
    """Boolean adjacency [M, M], zero diagonal."""
    beta = dtype(2.0 * noise_bound * np.sqrt(cbar2))
    adj = pair_gaps(a, b, dtype) < beta
    np.fill_diagonal(adj, False)
    return adj


def greedy_clique(adj):
    """The clique's members in the order they were appended."""
    adj = np.asarray(adj, bool)
    C = np.ones(len(adj), bool)
    clique = []
    while C.any():
        deg = np.where(C, (adj & C[None]).sum(1), -1)
        v = int(np.argmax(deg))
        clique.append(v)
        C &= adj[v]
    return clique


def clique_mask_words(clique):
    """The clique as 32 words, bit j of word w = correspondence 32 w + j (the layout of ``hp_teaser_register``)."""
    words = np.zeros(MAX_POINTS // 32, np.uint32)
    for v in clique:
        words[v // 32] |= np.uint32(1) << np.uint32(v % 32)
    return words


def _rotation(H, dtype):
    U, _, Vt = np.linalg.svd(H.astype(dtype))
    V = Vt.T
    D = np.diag(np.array([1.0, 1.0, np.linalg.det(V @ U.T)], dtype))
    return (V @ D @ U.T).astype(dtype)


def gnc_tls_rotation(am, bm, noise_bound_sq, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12, dtype=np.float64):
    """``R`` of ``bm ~ R am`` over the measurements [m, 3]; returns ``(R, weights)``."""
    am, bm = np.asarray(am, dtype), np.asarray(bm, dtype)
    nb2 = dtype(noise_bound_sq)
    w = np.ones(len(am), dtype)
    mu = dtype(1.0)
    cost_prev = dtype(np.inf)
    R = np.eye(3, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        for it in range(max_iterations):
            R = _rotation((am * w[:, None]).T @ bm, dtype)
            r2 = ((bm - am @ R.T) ** 2).sum(1)
            if it == 0:
                mu = dtype(1.0) / (dtype(2.0) * r2.max() / nb2 - dtype(1.0))
                if mu <= 0:
                    break
            cost = (w * r2).sum()
            th1, th2 = (mu + 1) / mu * nb2, mu / (mu + 1) * nb2
            w = np.where(r2 >= th1, 0.0, np.where(r2 <= th2, 1.0, np.sqrt(nb2 * mu * (mu + 1) / np.maximum(r2, 1e-300)) - mu)).astype(dtype)
            diff = abs(cost - cost_prev)
            cost_prev = cost
            mu = dtype(mu * dtype(gnc_factor))
            if diff < cost_threshold:
                break
    return R, w


def tls_translation(x, alpha, cbar2=1.0, dtype=np.float64):
    """Truncated least squares estimate of one coordinate from the values ``x`` [m]."""
    x = np.asarray(x, dtype)
    alpha = dtype(alpha)
    m = len(x)
    ends = np.empty(2 * m, dtype)
    ends[0::2], ends[1::2] = x - alpha, x + alpha
    ends = np.sort(ends, kind="stable")
    cand = dtype(0.5) * (ends[:-1] + ends[1:])
    S = np.abs(x[None] - cand[:, None]) <= alpha  # [2m - 1, m]
    cnt = S.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(cnt > 0, (S * x[None]).sum(1) / cnt, 0).astype(dtype)
        cost = (S * (x[None] - mean[:, None]) ** 2).sum(1) / (alpha * alpha) + (m - cnt) * dtype(cbar2)
    cost = np.where(cnt > 0, cost, np.inf)
    return mean[int(np.argmin(cost))]  # argmin: the lowest candidate of a tie


def register(a, b, noise_bound=0.01, cbar2=1.0, min_num_inliers=50, dtype=np.float64):
    """``dict(T [4,4], status, num_inliers, clique (sorted), clique_size)``; ``T`` is the identity when the status is not 0."""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    out = dict(T=np.eye(4, dtype=dtype), status=0, num_inliers=0, clique=[], clique_size=0)
    if len(a) == 0:
        out["status"] = -2
        return out
    adj = consistency_graph(a, b, noise_bound, cbar2, dtype)
    clique = sorted(greedy_clique(adj))
    out["clique"], out["clique_size"] = clique, len(clique)
    if len(clique) < 3:
        out["status"] = -2
        return out
    alpha = dtype(noise_bound * np.sqrt(cbar2))
    beta = dtype(2.0) * alpha
    ac, bc = a[clique], b[clique]
    R, _ = gnc_tls_rotation(ac[1:] - ac[:-1], bc[1:] - bc[:-1], beta * beta, dtype=dtype)
    x = bc - ac @ R.T
    t = np.array([tls_translation(x[:, k], alpha, cbar2, dtype) for k in range(3)], dtype)
    e = a @ R.T + t - b
    out["num_inliers"] = int((np.sqrt((e * e).sum(1)) < dtype(noise_bound)).sum())
    if out["num_inliers"] < min_num_inliers:
        out["status"] = -3
        return out
    out["T"][:3, :3], out["T"][:3, 3] = R, t
    return out


def correspondences(depth_rendered, depth_measured, K, mask_type="simple", depth_delta_thresh=0.1, dtype=np.float64):
    """The masked pixels in row-major order, back-projected from both depth maps: ``(a [N,3], b [N,3])``."""
    dr, dm, K = np.asarray(depth_rendered, dtype), np.asarray(depth_measured, dtype), np.asarray(K, dtype)
    mask = (dr > 0) & (dm > 0)
    if mask_type == "threshold":
        mask &= np.abs(dm - dr) <= dtype(depth_delta_thresh)
    elif mask_type != "simple":
        raise ValueError(f"Unknown mask type {mask_type}")
    v, u = np.nonzero(mask)

    def points(d):
        z = d[v, u]
        return np.stack([(u.astype(dtype) - K[0, 2]) * z / K[0, 0], (v.astype(dtype) - K[1, 2]) * z / K[1, 1], z], 1)

    return points(dr), points(dm)


def refine(depth_rendered, depth_measured, K, TCO, mask_type="simple", depth_delta_thresh=0.1, n_min_points=100, n_points=1000,
           noise_bound=0.01, min_num_inliers=50, use_farthest_point_sampling=True, dtype=np.float64):
    """One prediction: ``(TCO_refined [4,4], status, num_inliers, clique_size)``; the pose is returned unchanged unless the
    status is 0."""
    TCO = np.asarray(TCO, dtype)
    a, b = correspondences(depth_rendered, depth_measured, K, mask_type, depth_delta_thresh, dtype)
    N = len(a)
    if N < n_min_points:
        return TCO.copy(), -1, 0, 0
    M = min(n_points, N)
    idx = fps(a, M, dtype) if use_farthest_point_sampling else (np.arange(M) * N) // max(M, 1)
    r = register(a[idx], b[idx], noise_bound, 1.0, min_num_inliers, dtype)
    if r["status"] != 0:
        return TCO.copy(), r["status"], r["num_inliers"], r["clique_size"]
    return r["T"] @ TCO, 0, r["num_inliers"], r["clique_size"]


# ---- seeded inputs ---------------------------------------------------------------------------------------------------

def random_rotation(rs, max_angle):
    axis = rs.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rs.uniform(0.5, 1.0) * max_angle
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def make_registration_case(M, n_inliers, seed, extent=0.2, noise=1e-3, outlier=(0.05, 0.30), noise_bound=0.01, margin=0.0,
                           one_sided=False):
    """``a`` uniform in a cube of side ``extent``; ``b = R a + t`` + noise of norm <= ``noise`` for the first ``n_inliers`` (then
    shuffled), displaced by ``outlier[0] .. outlier[1]`` metres in a random direction for the rest.  Everything is rounded to
    float32 BEFORE it is returned, so that a float64 and a float32 consumer see the same numbers.  With ``margin > 0`` a point is
    redrawn until no pair it forms is within ``margin`` of the graph's threshold ``beta``.  ``one_sided``: the outliers are
    displaced towards -z only (an occluder in front of the object), which biases a plain least-squares fit.
    Returns ``(a, b, R, t, inlier_mask)``."""
    rs = np.random.RandomState(seed)
    R = random_rotation(rs, np.deg2rad(10.0))
    t = rs.uniform(-0.02, 0.02, 3)
    is_inlier = np.zeros(M, bool)
    is_inlier[rs.permutation(M)[:n_inliers]] = True
    beta = 2.0 * noise_bound
    a = np.zeros((M, 3), np.float32)
    b = np.zeros((M, 3), np.float32)

    def draw(inl):
        p = rs.uniform(-extent / 2, extent / 2, 3)
        d = rs.normal(size=3)
        d /= np.linalg.norm(d)
        if one_sided and not inl:
            d[2] = -abs(d[2])
        q = R @ p + t + d * (rs.uniform(0, noise) if inl else rs.uniform(*outlier))
        return p.astype(np.float32), q.astype(np.float32)

    for i in range(M):
        while True:
            a[i], b[i] = draw(is_inlier[i])
            if margin <= 0 or i == 0:
                break
            da = np.linalg.norm(a[:i].astype(np.float64) - a[i].astype(np.float64), axis=1)
            db = np.linalg.norm(b[:i].astype(np.float64) - b[i].astype(np.float64), axis=1)
            if (np.abs(np.abs(db - da) - beta) >= margin).all():
                break
    return a, b, R, t, is_inlier
