"""What the operations' DEFINITIONS fix, evaluated in numpy (float64) from the C ABI's outputs -- no line of `oracle/` is involved.

Every other GPU test compares the HIP path with `oracle/`, this repository's CPU restatement by the same hand; agreement there cannot
show that both read the algorithm right.  Here each operator of the stereo hot path is held against a second, independent statement
of what it computes, written from the published definitions (SURF: Bay et al. + the pattern tables of opencv_contrib's surf.cpp;
Lowe's ratio test; DLT triangulation; VO_utility.cpp:188-237 for the 3-D filter; PnP by its reprojection model):

  * the integral image is the double prefix sum, exactly;
  * a Hessian layer is the box-filter determinant dxx * dyy - 0.81 dxy^2 on the published box pattern, to float accuracy;
  * every SURF keypoint sits (within one sample, as its sub-sample interpolation allows) on a strict 3 x 3 x 3 maximum of those
    layers above the threshold, carries that determinant as its response and the sign of the trace as its class; the keypoints are
    the maxima (every comfortable numpy maximum whose own quadratic fit stays inside its cell is among them, at the fit's position);
    descriptor rows have unit length and |sum| <= sum|.| cell by cell;
  * the ratio matcher returns the pairs a float64 brute force returns, up to pairs whose ratio lies within 1e-5 of the threshold;
  * a triangulated point is the smallest right singular vector of the 4 x 4 DLT system (numpy SVD) and reprojects onto its two
    observations;
  * extract_3Dpoints keeps exactly the points the definition keeps (mean reprojection error below the tolerance, positive depth,
    depth within mean +- 3 sigma of those);
  * solvePnPRansac recovers a planted pose, and its inliers reproject within the threshold under it.

get_image, the preprocessing in front of the detectors, has its second statement in tests/preproc_definitions_np.py
(tests/test_gpu_preproc_definitions.py holds the HIP kernels to it); AKAZE and SIFT in tests/detector_definitions_np.py; the oriented and
the extended SURF branch (surf_orientation, surf_window_rotated, surf_descriptor) in tests/surf_oriented_np.py, held by
tests/test_gpu_surf_oriented_definitions.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DX = [(0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1)]
DY = [(2, 0, 7, 3, 1), (2, 3, 7, 6, -2), (2, 6, 7, 9, 1)]
DXY = [(1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1)]


def cv_round(x):
    return int(np.rint(x))                       # cvRound: to nearest, ties to even


def layer_size(octave, layer):
    return (9 + 6 * layer) << octave


def box_response(S, pattern, size, step, n_i, n_j):
    """sum over the pattern's boxes of (box sum) * weight / area for every sample whose template starts at (i * step, j * step)"""
    ratio = np.float32(size) / np.float32(9)
    out = np.zeros((n_i, n_j))
    for (x1, y1, x2, y2, wgt) in pattern:
        a, b, c, d = (cv_round(ratio * np.float32(v)) for v in (x1, y1, x2, y2))
        ys, xs = np.arange(n_i) * step, np.arange(n_j) * step
        box = (S[np.ix_(ys + b, xs + a)] + S[np.ix_(ys + d, xs + c)] - S[np.ix_(ys + b, xs + c)] - S[np.ix_(ys + d, xs + a)])
        out += box * (wgt / float((c - a) * (d - b)))
    return out


def det_trace_layer(S, h, w, octave, layer):
    """(det, trace, |dx dy| + 0.81 dxy^2) on the layer's sample grid (h / step x w / step), zero where the template does not fit"""
    step, size = 1 << octave, layer_size(octave, layer)
    rows, cols = h // step, w // step
    det, tr, mag = np.zeros((rows, cols)), np.zeros((rows, cols)), np.zeros((rows, cols))
    if size > h or size > w:
        return det, tr, mag
    n_i, n_j, m = 1 + (h - size) // step, 1 + (w - size) // step, (size // 2) // step
    dx, dy, dxy = (box_response(S, p, size, step, n_i, n_j) for p in (DX, DY, DXY))
    det[m:m + n_i, m:m + n_j] = dx * dy - 0.81 * dxy * dxy
    tr[m:m + n_i, m:m + n_j] = dx + dy
    mag[m:m + n_i, m:m + n_j] = np.abs(dx * dy) + 0.81 * dxy * dxy
    return det, tr, mag


@pytest.fixture(scope="module")
def image():
    from ergo_uvo_amd import synth
    return synth.stereo_pair(synth.Scene(77, 640), 0, 640, 360)[0]


@pytest.fixture(scope="module")
def uctx():
    import ergo_uvo_amd as uvo
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=1500), 0, 640, 360, 8192)
    yield c
    c.close()


def test_integral_is_the_double_prefix_sum(uctx, image):
    S = uctx.integral(image)
    want = np.zeros((361, 641), np.int64)
    want[1:, 1:] = np.cumsum(np.cumsum(image.astype(np.int64), 0), 1)
    assert np.array_equal(S, want)


def test_hessian_layers_are_the_box_filter_determinants(uctx, image):
    h, w = image.shape
    uctx.surf_detect(image)                                        # the debug hook reads the last image's integral
    S = np.zeros((h + 1, w + 1)); S[1:, 1:] = np.cumsum(np.cumsum(image.astype(np.float64), 0), 1)
    for octave in range(4):
        for layer in range(5):
            det, tr = uctx.hessian_layer((h, w), octave, layer)
            wd, wt, mag = det_trace_layer(S, h, w, octave, layer)
            # (dx, dy, dxy are sums of box means up to 255: their float error, ~1e-5, enters the products; responses of interest are > 1e3)
            assert np.all(np.abs(det - wd) <= 2e-5 * mag + 0.05), (octave, layer, np.abs(det - wd).max())
            assert np.all(np.abs(tr - wt) <= 1e-4 * (np.abs(wt) + 1.0)), (octave, layer)


def numpy_maxima(dets, traces, octave, thr, h, w, margin_rel):
    """findMaximaInLayer + interpolateKeypoint from the definition: strict 3x3x3 maxima of the three middle layers above thr (by
    `margin_rel` on both tests), quadratic fit; -> list of (x, y, size, response, laplacian sign)"""
    step = 1 << octave
    out = []
    for L in (1, 2, 3):
        size, size_lo, size_hi = layer_size(octave, L), layer_size(octave, L - 1), layer_size(octave, L + 1)
        if size_hi > h or size_hi > w:
            continue
        rows, cols = h // step, w // step
        m = (size_hi // 2) // step + 1
        d0, d1, d2 = dets[L - 1], dets[L], dets[L + 1]
        for i in range(m, rows - m):
            for j in np.nonzero(d1[i, m:cols - m] > thr * (1 + margin_rel))[0] + m:
                v = d1[i, j]
                nb = np.concatenate([d0[i - 1:i + 2, j - 1:j + 2].ravel(), d2[i - 1:i + 2, j - 1:j + 2].ravel(),
                                     np.delete(d1[i - 1:i + 2, j - 1:j + 2].ravel(), 4)])
                if not np.all(v > nb * (1 + margin_rel) + 1e-9):
                    continue
                N = np.stack([d0[i - 1:i + 2, j - 1:j + 2], d1[i - 1:i + 2, j - 1:j + 2], d2[i - 1:i + 2, j - 1:j + 2]])   # [layer][row][col]
                g = -np.array([(N[1, 1, 2] - N[1, 1, 0]) / 2, (N[1, 2, 1] - N[1, 0, 1]) / 2, (N[2, 1, 1] - N[0, 1, 1]) / 2])
                A = np.array([[N[1, 1, 0] - 2 * N[1, 1, 1] + N[1, 1, 2], (N[1, 2, 2] - N[1, 2, 0] - N[1, 0, 2] + N[1, 0, 0]) / 4, (N[2, 1, 2] - N[2, 1, 0] - N[0, 1, 2] + N[0, 1, 0]) / 4],
                              [0, N[1, 0, 1] - 2 * N[1, 1, 1] + N[1, 2, 1], (N[2, 2, 1] - N[2, 0, 1] - N[0, 2, 1] + N[0, 0, 1]) / 4],
                              [0, 0, N[0, 1, 1] - 2 * N[1, 1, 1] + N[2, 1, 1]]])
                A[1, 0], A[2, 0], A[2, 1] = A[0, 1], A[0, 2], A[1, 2]
                if abs(np.linalg.det(A)) < 1e-12:
                    continue
                x = np.linalg.solve(A, g)
                ci = step * (i - (size // 2) // step) + (size - 1) * 0.5
                cj = step * (j - (size // 2) // step) + (size - 1) * 0.5
                out.append((cj + x[0] * step, ci + x[1] * step, size + x[2] * (size - size_lo), v, traces[L][i, j] > 0, np.abs(x).max()))
    return out


def test_surf_keypoints_are_the_maxima_of_the_definition(uctx, image):
    h, w = image.shape
    thr = float(uctx.params.SURF_MIN_HESSIAN)
    kps, desc = uctx.surf_detect(image)
    assert len(kps) > 300
    S = np.zeros((h + 1, w + 1)); S[1:, 1:] = np.cumsum(np.cumsum(image.astype(np.float64), 0), 1)
    layers = {o: [det_trace_layer(S, h, w, o, l) for l in range(5)] for o in range(4)}
    # soundness: every keypoint's response is the determinant of a sample within one step of it, a 3x3x3 maximum above the threshold
    for kp in kps:
        o, step = int(kp["octave"]), 1 << int(kp["octave"])
        hit = False
        for L in (1, 2, 3):
            size = layer_size(o, L)
            det = layers[o][L][0]
            i0 = (kp["y"] - (size - 1) * 0.5) / step + (size // 2) // step
            j0 = (kp["x"] - (size - 1) * 0.5) / step + (size // 2) // step
            for i in range(int(np.floor(i0 - 1.01)), int(np.ceil(i0 + 1.01)) + 1):
                for j in range(int(np.floor(j0 - 1.01)), int(np.ceil(j0 + 1.01)) + 1):
                    if not (1 <= i < det.shape[0] - 1 and 1 <= j < det.shape[1] - 1):
                        continue
                    v = det[i, j]
                    if abs(v - kp["response"]) > 2e-4 * abs(v) + 1e-2:
                        continue
                    nb = np.concatenate([layers[o][L - 1][0][i - 1:i + 2, j - 1:j + 2].ravel(), layers[o][L + 1][0][i - 1:i + 2, j - 1:j + 2].ravel(),
                                         np.delete(det[i - 1:i + 2, j - 1:j + 2].ravel(), 4)])
                    slack = 1e-4 * layers[o][L][2][i - 1:i + 2, j - 1:j + 2].max() + 1e-2
                    if v > thr - slack and np.all(v > nb - slack):
                        hit = True
                        assert (kp["class_id"] > 0) == (layers[o][L][1][i, j] > 0) or abs(layers[o][L][1][i, j]) < 1e-2
        assert hit, kp
    # completeness: every comfortable maximum of the definition whose own fit stays inside its cell is a keypoint, where the fit puts it
    found = 0
    for o in range(4):
        dets, traces = [layers[o][l][0] for l in range(5)], [layers[o][l][1] for l in range(5)]
        for (x, y, size, v, lap, xmax) in numpy_maxima(dets, traces, o, thr, h, w, 1e-3):
            if xmax > 0.98:
                continue                                         # the fit leaves (or nearly leaves) the cell: interpolateKeypoint drops it
            d = np.hypot(kps["x"] - x, kps["y"] - y)
            k = int(np.argmin(d))
            assert d[k] < 0.05 and abs(kps["response"][k] - v) <= 2e-4 * abs(v) + 1e-2 and abs(kps["size"][k] - size) <= 0.51, (o, x, y, size, v, d[k], kps[k])
            found += 1
    assert found >= 0.9 * len(kps), (found, len(kps))
    # descriptor rows: unit length; per cell |sum dx| <= sum |dx|, |sum dy| <= sum |dy|
    assert np.abs(np.linalg.norm(desc.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    cells = desc.reshape(len(desc), 16, 4).astype(np.float64)
    assert np.all(np.abs(cells[:, :, 0]) <= cells[:, :, 2] + 1e-7) and np.all(np.abs(cells[:, :, 1]) <= cells[:, :, 3] + 1e-7)


def test_ratio_matcher_against_a_float64_brute_force(uctx):
    from ergo_uvo_amd import synth
    L, R = synth.stereo_pair(synth.Scene(78, 640), 0, 640, 360)
    _, d1 = uctx.surf_detect(L)
    _, d2 = uctx.surf_detect(R)
    ratio = float(uctx.params.LOWE_RATIO_THRESHOLD)
    got = uctx.match_features(d1, d2)
    a, b = d1.astype(np.float64), d2.astype(np.float64)
    D = np.sqrt(np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * a @ b.T, 0))
    order = np.argsort(D, axis=1)[:, :2]
    n1, n2 = D[np.arange(len(a)), order[:, 0]], D[np.arange(len(a)), order[:, 1]]
    want = {int(q): int(order[q, 0]) for q in range(len(a)) if n1[q] < ratio * n2[q]}
    have = {int(m["queryIdx"]): int(m["trainIdx"]) for m in got}
    assert len(have) == len(got) > 200
    undecided = {q for q in range(len(a)) if abs(n1[q] - ratio * n2[q]) <= 1e-5 * n2[q] or abs(n1[q] - n2[q]) <= 1e-6 * n2[q]}
    for q in set(want) ^ set(have):
        assert q in undecided, (q, n1[q], n2[q])
    for q in set(want) & set(have):
        assert want[q] == have[q] or q in undecided, q
    dist = {int(m["queryIdx"]): float(m["distance"]) for m in got}
    assert all(abs(dist[q] - n1[q]) <= 1e-5 * (1 + n1[q]) for q in have if q in want)
    assert list(got["queryIdx"]) == sorted(got["queryIdx"])      # knnMatch order: by query


def _rig_points(n, seed, noise):
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(1280)
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(2.5, 6, n)], 1)

    def proj(K, R, t, X):
        Y = X @ R.T + t
        return (Y[:, :2] / Y[:, 2:]) * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    x1 = (proj(rig.K_left, np.eye(3), np.zeros(3), X) + rng.normal(0, noise, (n, 2))).astype(np.float32)
    x2 = (proj(rig.K_right, rig.R_right, rig.t_right, X) + rng.normal(0, noise, (n, 2))).astype(np.float32)
    P1 = rig.K_left @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P2 = rig.K_right @ np.hstack([rig.R_right, rig.t_right[:, None]])
    return rig, X, x1, x2, P1, P2, proj


def test_triangulated_points_are_the_dlt_solution(uctx):
    rig, X, x1, x2, P1, P2, proj = _rig_points(400, 5, 0.4)
    Xh = uctx.triangulatePoints(P1, P2, x1, x2).astype(np.float64)          # 4 x n
    for k in range(0, 400, 7):
        A = np.stack([x1[k, 0] * P1[2] - P1[0], x1[k, 1] * P1[2] - P1[1], x2[k, 0] * P2[2] - P2[0], x2[k, 1] * P2[2] - P2[1]]).astype(np.float64)
        v = np.linalg.svd(A)[2][3]
        g = Xh[:, k] / np.linalg.norm(Xh[:, k])
        assert min(np.abs(g - v).max(), np.abs(g + v).max()) < 2e-5, k          # float output of a double SVD
    # noiseless observations: the point itself, and it reprojects onto both
    rig, X, x1, x2, P1, P2, proj = _rig_points(200, 6, 0.0)
    Xh = uctx.triangulatePoints(P1, P2, x1, x2).astype(np.float64)
    Xe = (Xh[:3] / Xh[3]).T
    assert np.abs(Xe - X).max() < 2e-2                                            # (pixel coordinates are float32)
    assert np.abs(proj(rig.K_left, np.eye(3), np.zeros(3), Xe) - x1).max() < 5e-2
    assert np.abs(proj(rig.K_right, rig.R_right, rig.t_right, Xe) - x2).max() < 5e-2


def test_extract_3dpoints_keeps_what_the_definition_keeps(uctx):
    """VO_utility.cpp:188-237: inhomogeneous point (float division), mean of the two reprojection errors < REPROJECTION_TOLERANCE and
    z > 0; then z within mean +- 3 sigma over those (math_utility.cpp:35-56: variance = E[z^2] - E[z]^2)."""
    tol = float(uctx.params.REPROJECTION_TOLERANCE)
    for n, noise, seed in ((800, 0.3, 3), (2500, 1.5, 4), (60, 0.2, 5)):
        rig, X, x1, x2, P1, P2, proj = _rig_points(n, seed, noise)
        p4 = uctx.triangulatePoints(P1, P2, x1, x2)
        p4[:, ::13] *= -1.0                                                        # sign flips leave the inhomogeneous point alone ...
        p4[2, 5::29] *= -1.0                                                       # ... a negated z puts the point behind the camera
        pts, idx = uctx.extract_3Dpoints(x1, x2, np.eye(3), np.zeros(3), rig.R_right, rig.t_right, rig.K_left, rig.K_right, p4)
        scale = np.where(p4[3] != 0, np.float32(1) / p4[3], np.float32(1))
        Xe = (p4[:3] * scale).T.astype(np.float64)
        e = 0.5 * (np.linalg.norm(proj(rig.K_left, np.eye(3), np.zeros(3), Xe) - x1, axis=1) + np.linalg.norm(proj(rig.K_right, rig.R_right, rig.t_right, Xe) - x2, axis=1))
        first = np.nonzero((e < tol) & (Xe[:, 2] > 0))[0]
        near = np.nonzero((np.abs(e - tol) < 1e-6) | (np.abs(Xe[:, 2]) < 1e-9))[0]
        assert len(near) == 0                                                      # (no borderline point in these draws)
        z = Xe[first, 2]
        mean, sd = z.mean(), np.sqrt((z * z).mean() - z.mean() ** 2)
        edge = np.minimum(np.abs(z - (mean + 3 * sd)), np.abs(z - (mean - 3 * sd))) < 1e-9
        assert not edge.any()
        want = first[(z <= mean + 3 * sd) & (z >= mean - 3 * sd)]
        assert np.array_equal(idx, want), (n, len(idx), len(want))
        assert np.array_equal(pts, Xe[want])


def test_pnp_ransac_recovers_a_planted_pose(uctx):
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(1280)
    rng = np.random.default_rng(9)
    n = 1500
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(2.5, 6, n)], 1)
    rvec_t, t_t = np.array([0.012, -0.02, 0.007]), np.array([0.04, -0.015, 0.06])
    Rm = uctx.Rodrigues(rvec_t)
    th = np.linalg.norm(rvec_t); k = rvec_t / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    assert np.abs(Rm - (np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx)).max() < 1e-12          # Rodrigues, by its formula
    Y = X @ Rm.T + t_t
    x = (Y[:, :2] / Y[:, 2:]) * np.array([rig.K_left[0, 0], rig.K_left[1, 1]]) + np.array([rig.K_left[0, 2], rig.K_left[1, 2]])
    x += rng.normal(0, 0.3, x.shape)
    bad = rng.choice(n, 300, replace=False)
    x[bad] += rng.uniform(20, 60, (300, 2)) * rng.choice([-1, 1], (300, 2))
    thr = float(uctx.params.REPROJECTION_ERROR_THRESHOLD)
    ok, rvec, tvec, inl = uctx.solvePnPRansac(X, x.astype(np.float32), rig.K_left)
    assert ok and np.abs(rvec - rvec_t).max() < 2e-3 and np.abs(tvec - t_t).max() < 1e-2
    assert not set(inl.tolist()) & set(bad.tolist()) and len(inl) > 0.9 * (n - 300)
    Rr = uctx.Rodrigues(rvec)
    Yr = X[inl] @ Rr.T + tvec
    xr = (Yr[:, :2] / Yr[:, 2:]) * np.array([rig.K_left[0, 0], rig.K_left[1, 1]]) + np.array([rig.K_left[0, 2], rig.K_left[1, 2]])
    err = np.linalg.norm(xr - x[inl].astype(np.float32), axis=1)
    assert np.mean(err <= thr) > 0.99 and err.max() < 1.5 * thr            # the inlier set is the best hypothesis', the pose its refit


def test_essential_matrix_and_recovered_pose_by_their_definitions(uctx):
    """findEssentialMat / recoverPose (VO_utility.cpp:134-180): E is an essential matrix (rank 2, two equal singular values:
    2 E E^T E = tr(E E^T) E), its inliers satisfy the epipolar constraint within the threshold, and the recovered (R, t) is a
    rotation, a unit translation, and the planted motion."""
    from ergo_uvo_amd import synth
    rig = synth.stereo_rig(1280)
    K = rig.K_left
    rng = np.random.default_rng(21)
    n = 600
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(2.5, 7, n)], 1)
    R_t = uctx.Rodrigues(np.array([0.02, -0.03, 0.01]))
    t_t = np.array([0.12, -0.03, 0.05])

    def proj(R, t):
        Y = X @ R.T + t
        return (Y[:, :2] / Y[:, 2:]) * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    p1 = proj(np.eye(3), np.zeros(3)) + rng.normal(0, 0.2, (n, 2))
    p2 = proj(R_t, t_t) + rng.normal(0, 0.2, (n, 2))
    bad = rng.choice(n, 120, replace=False)
    p2[bad] += rng.uniform(15, 40, (120, 2)) * rng.choice([-1, 1], (120, 2))
    p1, p2 = p1.astype(np.float32), p2.astype(np.float32)
    thr = 1.0
    ok, E, mask = uctx.findEssentialMat(p1, p2, K, method=8, prob=0.999, threshold=thr, max_iters=2000)
    assert ok
    E = E / np.linalg.norm(E)
    sv = np.linalg.svd(E, compute_uv=False)
    assert sv[2] < 1e-7 and abs(sv[0] - sv[1]) < 1e-7
    assert np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max() < 1e-7
    Ki = np.linalg.inv(K)
    h1 = np.c_[p1.astype(np.float64), np.ones(n)] @ Ki.T
    h2 = np.c_[p2.astype(np.float64), np.ones(n)] @ Ki.T
    # Sampson distance in pixels^2 (focal ~ K[0,0]) of the pairs the mask keeps
    Ex1, Etx2 = h1 @ E.T, h2 @ E
    samp = (np.sum(h2 * Ex1, 1) ** 2) / (Ex1[:, 0] ** 2 + Ex1[:, 1] ** 2 + Etx2[:, 0] ** 2 + Etx2[:, 1] ** 2) * K[0, 0] ** 2
    inl = mask.astype(bool)
    assert inl.sum() > 0.9 * (n - 120) and not inl[bad].any()
    assert np.all(samp[inl] <= thr * thr * 1.02)
    good, R, t, m2 = uctx.recoverPose(E, p1, p2, K, mask)
    assert abs(np.linalg.det(R) - 1) < 1e-9 and np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.norm(t) - 1) < 1e-9
    # (the cheirality count also drops points triangulated beyond distanceThresh = 50 baselines: the planted baseline is 0.135 of a unit)
    assert good == int((m2 > 0).sum()) and good > 0.5 * inl.sum() and not np.any((m2 > 0) & ~inl)
    assert np.abs(R - R_t).max() < 5e-3 and np.abs(t.ravel() - t_t / np.linalg.norm(t_t)).max() < 5e-2


# ------------------------------------------------------------------------------------------------------------------------------------
# Round 5: the three operators whose restatement is the most intricate, against tests/definitions_np.py (numpy float64, written from
# the published definitions; imports nothing of oracle/): the 64-float descriptor, EPnP inside solvePnPRansac, findHomography's mask.

def _descriptor_ties(img, kp, eps=2e-4):
    """21 x 21 cells of the keypoint's area-averaged window whose exact average lies within eps of k + 0.5: the 8-bit rounding of such a
    cell is decided by the resize's own arithmetic (float weights; 2 x 2 blocks round half up), not by the definition."""
    import definitions_np as D
    win, n = D.surf_window(img, kp["x"], kp["y"], kp["size"])
    W = D.area_weights(n, 21)
    v = W @ win @ W.T
    return int((np.abs(v - np.floor(v) - 0.5) < eps).sum())


@pytest.mark.parametrize("shape,seed,thr,min_kps,min_clean", [((360, 640), 77, 1500, 600, 300), ((1080, 1920), None, 6387, 2800, 1500)])
def test_surf64_descriptor_against_its_definition(shape, seed, thr, min_kps, min_clean):
    """VO_utility.cpp:114-119 -> SURF::detectAndCompute, descriptor half: every row of uvo_surf_detect against the numpy statement of
    the upright 64-float descriptor (window floor(21 * size * 1.2 / 9) clamped to the image, exact area average to 21 x 21 with the
    8-bit rounding, 20 x 20 Haar differences, sigma = 3.3 Gaussian, 4 x 4 cells, unit length).  Keypoints none of whose 441 cells sits
    on a rounding tie must agree to 1e-6 per element (float accuracy of a 64-float row); the others -- a grey level either way in a
    few cells -- to 6e-3, and 97 % of ALL keypoints to 2e-3.  1080p: windows up to several hundred pixels (most above 128)."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import definitions_np as D
    import ergo_uvo_amd as uvo
    from ergo_uvo_amd import synth
    h, w = shape
    img = synth.stereo_pair(synth.Scene(synth.SEEDS["C3"] if seed is None else seed, w), 0, w, h)[0]
    c = uvo.Context(uvo.Params.stereo(SURF_MIN_HESSIAN=thr), 0, w, h, 8192)
    try:
        kps, desc = c.surf_detect(img)
    finally:
        c.close()
    assert len(kps) >= min_kps
    err = np.array([np.abs(D.surf64_upright(img, kp["x"], kp["y"], kp["size"]) - desc[k].astype(np.float64)).max() for k, kp in enumerate(kps)])
    ties = np.array([_descriptor_ties(img, kp) for kp in kps])
    wins = np.floor(np.float32(21) * (kps["size"] * np.float32(1.2) / np.float32(9))).astype(int)
    clean = ties == 0
    assert clean.sum() >= min_clean, clean.sum()
    assert err[clean].max() <= 1e-6, (err[clean].max(), int(np.argmax(np.where(clean, err, 0))))
    assert err.max() <= 6e-3 and np.mean(err <= 2e-3) >= 0.97, (err.max(), np.mean(err <= 2e-3))
    if h >= 1080:
        big = clean & (wins > 128)
        assert big.sum() >= 50 and err[big].max() <= 1e-6, (big.sum(), wins.max())


def _dyadic_pnp_case(n, seed, R, t, K):
    """Exactly consistent float32 data for a planted pose: camera-frame depths are powers of two and x / y multiples of Z / 128, K has integer
    focal lengths, R is a signed permutation (the only rotations with dyadic entries) -- object points, image points and pose are then
    all exactly representable, so an exact solver must return the pose to rounding error of its own arithmetic."""
    rng = np.random.default_rng(seed)
    Z = rng.choice([2.0, 4.0, 8.0], n)
    Y = np.stack([rng.integers(-64, 65, n) / 64.0 * Z * 0.5, rng.integers(-40, 41, n) / 64.0 * Z * 0.5, Z], 1)
    X = (Y - t) @ R
    x = (Y[:, :2] / Y[:, 2:]) * np.array([K[0, 0], K[1, 1]]) + np.array([K[0, 2], K[1, 2]])
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X) and np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return X, x.astype(np.float32)


def test_epnp_recovers_exact_poses_and_its_refit_is_near_the_least_squares_optimum(uctx):
    """cv::solvePnPRansac(..., SOLVEPNP_EPNP) (visual_odometry.h:647-648).  (i) Noise-free, exactly representable data: five points (the
    single solve OpenCV does when npoints == model_points), six (the smallest RANSAC case) and N points -- RANSAC + the refit on all
    inliers -- recover the planted pose to 1e-9 (observed ~1e-14), every point an inlier.  (ii) Noisy N points: the returned pose's
    reprojection RMS over its inliers is within 2 % of the RMS after a Levenberg-Marquardt polish of that pose (scipy) -- EPnP is not
    the maximum-likelihood estimator, but a correct one lands next to it (observed 1.0004 .. 1.004)."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import definitions_np as D
    K = np.array([[700.0, 0, 640], [0, 700, 360], [0, 0, 1]])
    Rz = np.array([[0., -1, 0], [1, 0, 0], [0, 0, 1]])
    Rx = np.array([[1., 0, 0], [0, 0, -1], [0, 1, 0]])
    t = np.array([0.25, -0.125, 0.5])
    for name, R in (("identity", np.eye(3)), ("90 degrees about z", Rz), ("90 degrees about x", Rx)):
        for n in (5, 6, 40, 400, 3000):
            X, x = _dyadic_pnp_case(n, 3 + n, R, t, K)
            ok, rvec, tvec, inl = uctx.solvePnPRansac(X, x, K)
            assert ok and len(inl) == n and np.array_equal(inl, np.arange(n)), (name, n, len(inl))
            assert np.abs(D.rodrigues(rvec) - R).max() <= 1e-9 and np.abs(tvec - t).max() <= 1e-9, (name, n, rvec, tvec)
    rng = np.random.default_rng(11)
    for n, noise in ((300, 0.3), (1500, 0.5), (60, 0.2), (3000, 0.4)):
        X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(2.5, 6, n)], 1).astype(np.float32).astype(np.float64)
        rv, tt = np.array([0.012, -0.02, 0.007]), np.array([0.04, -0.015, 0.06])
        x = (D.project(X, rv, tt, K) + rng.normal(0, noise, (n, 2))).astype(np.float32)
        ok, rvec, tvec, inl = uctx.solvePnPRansac(X, x, K, reprojection_error=8.0)
        assert ok and len(inl) >= 0.98 * n
        Xi, xi = X[inl], x[inl].astype(np.float64)
        rms = D.reprojection_rms(Xi, xi, rvec, tvec, K)
        rp, tp = D.pose_polish(Xi, xi, rvec, tvec, K)
        best = D.reprojection_rms(Xi, xi, rp, tp, K)
        assert best <= rms <= 1.02 * best, (n, noise, rms, best)
        assert np.abs(rvec - rv).max() < 5e-3 and np.abs(tvec - tt).max() < 2e-2


@pytest.mark.parametrize("n,n_out,noise,thr,seed", [(250, 50, 0.3, 1.0, 1), (800, 300, 0.5, 2.0, 2), (60, 10, 0.2, 1.0, 3), (400, 80, 0.05, 0.1, 4), (3000, 900, 0.4, 1.0, 5)])
def test_find_homography_mask_is_that_of_a_four_point_model_of_the_replayed_stream(uctx, n, n_out, noise, thr, seed):
    """cv::findHomography(RANSAC) (VO_utility.cpp:152): the mask it returns is the inlier set -- squared reprojection distance <=
    threshold^2 -- of ONE of the 4-point models RANSAC fits, and RANSAC's subsets are fixed by cv::RNG((uint64)-1).  The stream, the
    draws (redraw on a duplicate) and the normalised DLT are restated in numpy; the test finds the subset of the stream whose model's
    inlier set IS the mask (up to pairs within 0.1 % of the threshold), checks that no earlier subset's model had more inliers (RANSAC
    keeps the first best), and that no planted outlier is in."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import definitions_np as D
    rng = np.random.default_rng(seed)
    H0 = np.array([[1.02, 0.03, 12.0], [-0.02, 0.97, -7.0], [2e-5, -1e-5, 1.0]])
    p = np.stack([rng.uniform(20, 1260, n), rng.uniform(20, 700, n)], 1)
    ph = np.c_[p, np.ones(n)] @ H0.T
    q = ph[:, :2] / ph[:, 2:] + rng.normal(0, noise, (n, 2))
    bad = rng.choice(n, n_out, replace=False)
    q[bad] += rng.uniform(15, 50, (n_out, 2)) * rng.choice([-1, 1], (n_out, 2))
    p, q = p.astype(np.float32), q.astype(np.float32)
    ok, H, mask = uctx.findHomography(p, q, method=8, threshold=thr, max_iters=2000, confidence=0.995)
    inl = mask.astype(bool)
    assert ok and not inl[bad].any() and inl.sum() >= 0.5 * (n - n_out)
    hit, counts = None, []
    for k, s in enumerate(D.ransac_subsets(n, 4, 400)):
        Hk = D.homography_dlt(p[s], q[s])
        e = D.homography_err2(Hk, p, q) if np.all(np.isfinite(Hk)) else np.full(n, np.inf)
        lo, hi = e <= thr * thr * (1 - 1e-3), e <= thr * thr * (1 + 1e-3)
        counts.append(int(lo.sum()))
        if np.all(inl[lo]) and not np.any(inl[~hi]):
            hit = k
            break
    assert hit is not None, "no 4-point model of the first 400 subsets of cv::RNG((uint64)-1) has the returned mask as its inlier set"
    assert counts[hit] + 2 >= max(counts), (hit, counts[hit], max(counts))           # RANSAC keeps the FIRST model with the most inliers
    # the refined H (refit on the inliers + LM) explains the inliers at least as well as the 4-point model did
    assert np.sqrt(D.homography_err2(H / H[2, 2], p[inl], q[inl]).mean()) <= np.sqrt(D.homography_err2(Hk, p[inl], q[inl]).mean()) + 1e-9
