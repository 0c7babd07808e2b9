"""Register a reconstructed cloud to a ground-truth cloud before it is scored (eval_cloud --register).

A COLMAP reconstruction lives in an arbitrary frame (rotation, translation and scale are gauge freedoms of structure from motion),
a laser scan in the scanner's.  Three steps bring one into the other, as the Tanks and Temples protocol does:

    init_from_cameras        a similarity from the camera centres of two COLMAP models of the same images, matched by image name
    ops.cloud_voxel_downsample   both clouds thinned to one point per voxel, so that point density does not steer the fit
    register                 trimmed ICP in stages of decreasing distance: point-to-point, or point-to-plane over the normals
                             a fused cloud carries (icp='plane')

The search (ops.cloud_grid / cloud_nearest), the move (ops.cloud_transform), the reduction of the matched pairs to 18 sums
(ops.cloud_pair_moments) and the down-sampling run on the device; per iteration only 19 words cross to the host, where the
closed form of Umeyama / Horn turns them into a 4x4 matrix in float64 (similarity_from_moments).  Point-to-plane reduces the
pairs to 37 sums instead (ops.cloud_plane_moments; 38 words cross), and a 6x6 or 7x7 solve turns them into an increment of the
matrix (motion_from_plane_moments).  The planes are the source's (a fused cloud's own normals) or the target's
(normal_side='target': the ground truth's normals, given or estimated by ops.cloud_knn + ops.cloud_normals, for a reconstruction
that carries none; ops.cloud_plane_moments_target).

Without cameras or a matrix, global_init (register's init='global'; eval_cloud --register_global) finds
the start from the clouds alone: FPFH descriptors of both down-sampled clouds (ops.cloud_fpfh), matched exactly in feature space
(ops.cloud_feature_nearest), three-point hypotheses over the matches scored on the device (ops.cloud_ransac), the best few verified
against the whole down-sampled clouds.  This module imports without a GPU; only `register` and `global_init` need one.  Not here:
orienting normals by propagation, a symmetric objective, Fast Global Registration and a learned descriptor.
"""
import numpy as np

from . import colmap

DEFAULT_DISTANCES = (2.0, 1.0, 0.5)          # 4x, 2x, 1x eval_cloud's largest default tolerance: a default, not a measurement
RANK_TOLERANCE = 1e-10                       # second / first singular value of the cross-covariance below this: collinear pairs;
                                             # smallest / largest eigenvalue of the point-to-plane system below this: free motion


def similarity_from_moments(count, moments, pivot_src=None, pivot_dst=None, with_scale=False):
    """The least-squares similarity b ~ s R a + t of `count` pairs from their 18 sums (ops.cloud_pair_moments' layout: sum a (3),
    sum b (3), sum a_r b_c (9), sum |a|^2, sum |b|^2, sum d2) with a = source - pivot_src, b = target - pivot_dst -> 4x4 float64.
    Umeyama's closed form: cross-covariance sum(a b^T) / k - mean(a) mean(b)^T, its 3x3 SVD, the determinant fix (never a
    reflection), s = tr(D E) / var(a) when with_scale else 1, t from the centroids.  ValueError for fewer than 3 pairs or a
    cross-covariance of rank < 2 (collinear pairs): the fit is not determined."""
    k = int(count)
    m = np.asarray(moments, np.float64).reshape(-1)
    if m.shape != (18,):
        raise ValueError('moments: expected 18 sums, got %d' % m.size)
    if k < 3:
        raise ValueError('%d pairs: a similarity needs at least 3' % k)
    ps = np.zeros(3) if pivot_src is None else np.asarray(pivot_src, np.float64).reshape(3)
    pd = np.zeros(3) if pivot_dst is None else np.asarray(pivot_dst, np.float64).reshape(3)
    ma, mb = m[0:3] / k, m[3:6] / k
    cov = m[6:15].reshape(3, 3) / k - np.outer(ma, mb)          # cov[r][c] = cov(a_r, b_c)
    var_a = m[15] / k - float(ma @ ma)
    U, D, Vt = np.linalg.svd(cov.T)                              # cov^T = sum (b - mb)(a - ma)^T / k = U D V^T
    if not (D[0] > 0.0 and D[1] > RANK_TOLERANCE * D[0]):
        raise ValueError('the %d pairs are collinear (singular values %s): the fit is not determined' % (k, D.tolist()))
    E = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        E[2] = -1.0
    R = (U * E) @ Vt
    s = 1.0
    if with_scale:
        if not var_a > 0.0:
            raise ValueError('the source pairs have no extent: the scale is not determined')
        s = float((D * E).sum()) / var_a
    T = np.eye(4)
    T[:3, :3] = s * R
    T[:3, 3] = (pd + mb) - s * (R @ (ps + ma))
    return T


def similarity_from_points(P, Q, with_scale=False):
    """The same from explicit correspondences: P (k,3) -> Q (k,3), float64."""
    P, Q = np.asarray(P, np.float64).reshape(-1, 3), np.asarray(Q, np.float64).reshape(-1, 3)
    if P.shape != Q.shape:
        raise ValueError('P %s and Q %s: one target per source point' % (P.shape, Q.shape))
    if len(P) < 3:
        raise ValueError('%d pairs: a similarity needs at least 3' % len(P))
    ps, pd = P.mean(axis=0), Q.mean(axis=0)
    a, b = P - ps, Q - pd
    m = np.concatenate([a.sum(0), b.sum(0), (a[:, :, None] * b[:, None, :]).sum(0).reshape(-1),
                        [(a * a).sum(), (b * b).sum(), ((Q - P) ** 2).sum()]])
    return similarity_from_moments(len(P), m, ps, pd, with_scale)


def _exp_so3(w):
    """Rodrigues' formula: the rotation Exp(w) of the rotation vector w (3,), orthonormal to rounding for every |w|."""
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    theta = float(np.sqrt(w @ w))
    if theta < 1e-8:                                             # sin t / t and (1 - cos t) / t^2 to within 1e-17 of their limits
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(theta) / theta) * K + ((1.0 - np.cos(theta)) / (theta * theta)) * (K @ K)


def motion_from_plane_moments(count, moments, pivot=None, with_scale=False, extent=1.0):
    """One Gauss-Newton step of point-to-plane ICP from the 37 sums of `count` pairs (ops.cloud_plane_moments' layout: sum J_a J_b
    for a <= b row-major (28), sum J_a r (7), sum r^2, sum d2; J = [g x n' (3), n' (3), q . n']) -> the 4x4 float64 increment
    D: the current matrix T becomes D T.  The normal equations (sum J J^T) x = -sum J r are solved for x = (omega, t) (6 unknowns)
    or (omega, t, sigma) (7, with_scale), and D is the EXACT motion x -> pivot + (1 + sigma) Exp(omega) (x - pivot) + t (Rodrigues'
    formula), so the rotation stays orthonormal however many increments are composed.  extent: a length of the scene (register
    passes half the diagonal of the target's box); the rotational and scale columns are divided by it before the system is judged
    and solved, so that rotations and translations share a unit.  ValueError for fewer pairs than unknowns, and when the system's
    smallest eigenvalue is below RANK_TOLERANCE of its largest: the pairs do not constrain the motion."""
    k = int(count)
    m = np.asarray(moments, np.float64).reshape(-1)
    if m.shape != (37,):
        raise ValueError('moments: expected 37 sums, got %d' % m.size)
    dim = 7 if with_scale else 6
    if k < dim:
        raise ValueError('%d pairs: a point-to-plane step with %d unknowns needs at least %d' % (k, dim, dim))
    extent = float(extent)
    if not (extent > 0.0 and np.isfinite(extent)):
        raise ValueError('extent must be positive and finite, got %r' % (extent,))
    p = np.zeros(3) if pivot is None else np.asarray(pivot, np.float64).reshape(3)
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = m[:28]
    A = A + np.triu(A, 1).T
    unit = np.array([extent] * 3 + [1.0] * 3 + [extent])[:dim]
    A, b = A[:dim, :dim] / np.outer(unit, unit), m[28:28 + dim] / unit
    eig = np.linalg.eigvalsh(A)
    if not (eig[-1] > 0.0 and eig[0] > RANK_TOLERANCE * eig[-1]):
        raise ValueError('the %d pairs do not constrain the motion (eigenvalues of the point-to-plane system %s): a single plane '
                         "leaves sliding along it free; use icp='point'" % (k, eig.tolist()))
    x = np.linalg.solve(A, -b) / unit
    s = 1.0 + float(x[6]) if with_scale else 1.0
    if not s > 0.0:
        raise ValueError('the point-to-plane step asks for the scale factor %r: the pairs do not constrain the motion' % s)
    D = np.eye(4)
    D[:3, :3] = s * _exp_so3(x[:3])
    D[:3, 3] = (p + x[3:6]) - D[:3, :3] @ p
    return D


def apply(T, points):
    """points (k,3) float64 through the 4x4 T, in float64 (host helper; the device form is ops.cloud_transform)."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    return np.asarray(points, np.float64) @ T[:3, :3].T + T[:3, 3]


def camera_centres(model):
    """(N,3) float64: -R^T t of every image of a colmap.Model."""
    return -np.einsum('nji,nj->ni', model.R, model.t)


def cameras_from_models(recon_sparse_dir, gt_sparse_dir):
    """Two COLMAP sparse model folders of the same images -> (P, Q) (k,3) float64: the camera centres of the images both list, by
    NAME, in the first and in the second model's frame.  Only poses are used, so cameras of any model but FOV are read
    (colmap.read_model(allow_distorted=True)): ETH3D's own calibration folder (THIN_PRISM_FISHEYE) serves as the second."""
    a, b = colmap.read_model(recon_sparse_dir, allow_distorted=True), colmap.read_model(gt_sparse_dir, allow_distorted=True)
    at = dict(zip(b.names, range(len(b.names))))
    pairs = [(i, at[name]) for i, name in enumerate(a.names) if name in at]
    return camera_centres(a)[[i for i, _ in pairs]].reshape(-1, 3), camera_centres(b)[[j for _, j in pairs]].reshape(-1, 3)


def init_from_cameras(recon_sparse_dir, gt_sparse_dir):
    """Two COLMAP sparse model folders (colmap.read_model: text or binary) of the same images, the first in the reconstruction's
    frame, the second in the ground truth's -> (4x4 similarity moving the first frame into the second, number of images matched
    by NAME, rms distance of the matched camera centres after it).  ValueError when fewer than 3 names match or the matched
    centres are collinear (a straight camera path leaves the rotation about it free)."""
    P, Q = cameras_from_models(recon_sparse_dir, gt_sparse_dir)
    if len(P) < 3:
        raise ValueError('%s and %s have %d image names in common: at least 3 are needed' % (recon_sparse_dir, gt_sparse_dir, len(P)))
    try:
        T = similarity_from_points(P, Q, with_scale=True)
    except ValueError as e:
        raise ValueError('the %d matched camera centres do not determine a similarity: %s' % (len(P), e))
    rms = float(np.sqrt(((apply(T, P) - Q) ** 2).sum(axis=1).mean()))
    return T, len(P), rms


def box_corners(lo, hi):
    """The eight corners (8,3) of the box lo .. hi."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    return np.array([[(lo, hi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)], np.float64)


def corner_move(T0, T1, corners):
    """The largest distance any corner moves between the matrices T0 and T1."""
    d = apply(T1, corners) - apply(T0, corners)
    return float(np.sqrt((d * d).sum(axis=1)).max())


def _pair_of(value, name):
    """One positive number for both clouds, or (source's, target's) -> a tuple of two floats."""
    pair = tuple(float(v) for v in value) if np.ndim(value) else (float(value), float(value))
    if len(pair) != 2 or any(not (v > 0.0 and np.isfinite(v)) for v in pair):
        raise ValueError('%s: expected a positive number or (source, target), got %r' % (name, value))
    return pair


def global_init(recon, gt, with_scale=False, voxel=None, feature_voxel=None, normal_k=16, feature_k=32, feature_radius=None, tau=None,
                hypotheses=65536, seed=0, mutual=True, edge_ratio=0.9, best=4, device=None):
    """A starting matrix for `register` from the clouds alone: recon (M,3) and gt (N,3) (host arrays or device tensors, float32),
    however far apart, -> dict.  On the device, in this order:

      1  both clouds are thinned by ops.cloud_voxel_downsample to feature_voxel (a number, or (source's, target's)); None: twice
         `voxel`, the registration's; with_scale: 1/64 of each cloud's OWN bounding-box diagonal (ops.cloud_bounds), since a
         length means nothing across two clouds of unknown scale -- which presumes that both cover about the same extent;
      2  per cloud one ops.cloud_grid of feature_radius (None: 5 feature voxels), ops.cloud_knn in itself, and unoriented normals
         from the first normal_k neighbours (ops.cloud_normals, self_counts=True);
      3  FPFH over the first feature_k neighbours (ops.cloud_fpfh);
      4  every source descriptor finds its nearest target descriptor (ops.cloud_feature_nearest); mutual: the pairs whose target
         finds that source back are kept, unless fewer than a third survive (then all are kept, as Open3D does);
      5  `hypotheses` triples of matches drawn by numpy.random.Generator(PCG64(seed)), on the host;
      6  ops.cloud_ransac: the `best` hypotheses by the number of matches within tau (None: 1.5 of the target's feature voxels; in
         the target's units), pruned by edge_ratio;
      7  each of them moves the whole down-sampled source (ops.cloud_transform), which is searched in a grid of radius tau over
         the down-sampled target (ops.cloud_nearest, ops.cloud_counts): its fitness is the share of source points within tau;
      8  the highest fitness wins, RANSAC's order on ties.

    -> matrix (4x4 nested lists: moves recon towards gt), fitness, scale, candidates [{index, count, sum, fitness}], n_recon /
    n_gt (points after step 1), n_recon_normals / n_gt_normals (usable normals), n_recon_features / n_gt_features (descriptors
    that are not zero), n_matches, n_mutual (None without mutual), mutual_used, n_valid_hypotheses, seed, and every parameter as
    it was used (feature_voxel, feature_radius: pairs).  ValueError naming the step when fewer than 3 matches remain or no
    hypothesis is valid.  Every default is a default, not a measurement."""
    import torch
    from .. import ops
    if voxel is None and feature_voxel is None and not with_scale:
        raise ValueError('global_init: give voxel (the registration\'s) or feature_voxel')
    for value, name, lo, hi in ((normal_k, 'normal_k', 2, 32), (feature_k, 'feature_k', 1, 32), (hypotheses, 'hypotheses', 1, 1 << 24),
                                (best, 'best', 1, 8), (seed, 'seed', 0, (1 << 63) - 1)):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
            raise ValueError('%s: expected an integer in %d..%d, got %r' % (name, lo, hi, value))
    if not 0.0 < float(edge_ratio) <= 1.0:
        raise ValueError('edge_ratio must be in (0, 1], got %r' % (edge_ratio,))
    if tau is not None and not (float(tau) > 0.0 and np.isfinite(float(tau))):
        raise ValueError('tau must be positive and finite, got %r' % (tau,))
    if feature_voxel is not None:
        fv = _pair_of(feature_voxel, 'feature_voxel')
    elif not with_scale:
        fv = _pair_of(2.0 * float(voxel), 'voxel')
    radius_given = None if feature_radius is None else _pair_of(feature_radius, 'feature_radius')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

    def upload(x):
        if isinstance(x, torch.Tensor):
            return x.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1, 3))).to(dev)

    def describe(cloud, edge, radius):
        down = ops.cloud_voxel_downsample(cloud, edge)[0].contiguous()
        knn = ops.cloud_knn(ops.cloud_grid(down, radius), down, max(int(normal_k), int(feature_k)), exclude_same_index=True)[1]
        nrm = ops.cloud_normals(down, down, knn[:, :int(normal_k)].contiguous(), self_counts=True)     # the first k of a longer list
        feat = ops.cloud_fpfh(down, knn[:, :int(feature_k)].contiguous(), nrm)
        return down, int((nrm != 0).any(dim=1).sum().item()), feat, int((feat != 0).any(dim=1).sum().item())

    with torch.cuda.device(dev):
        src, dst = upload(recon), upload(gt)
        if feature_voxel is None and with_scale:
            boxes = [ops.cloud_bounds(c) for c in (src, dst)]
            if any(lo is None for lo, _ in boxes):
                raise ValueError('global_init: a cloud has no finite point')
            fv = _pair_of([float(np.sqrt(((hi - lo) ** 2).sum())) / 64.0 for lo, hi in boxes], 'the clouds\' extent')
        radius = radius_given or (5.0 * fv[0], 5.0 * fv[1])
        tau = 1.5 * fv[1] if tau is None else float(tau)
        src, n_src_normals, f_src, n_src_feat = describe(src, fv[0], radius[0])
        dst, n_dst_normals, f_dst, n_dst_feat = describe(dst, fv[1], radius[1])
        fwd = ops.cloud_feature_nearest(f_dst, f_src)[1].long()
        rows = torch.nonzero(fwd >= 0).reshape(-1)
        n_matches, n_mutual, mutual_used = int(rows.numel()), None, False
        if mutual and n_matches:
            back = ops.cloud_feature_nearest(f_src, f_dst)[1].long()
            agree = rows[back[fwd[rows]] == rows]
            n_mutual = int(agree.numel())
            if 3 * n_mutual >= n_matches:
                rows, mutual_used = agree, True
        if int(rows.numel()) < 3:
            raise ValueError('global_init: the feature matching left %d matches (%d source and %d target descriptors): at least 3 '
                             'are needed' % (int(rows.numel()), n_src_feat, n_dst_feat))
        a, b = src[rows].contiguous(), dst[fwd[rows]].contiguous()
        triples = np.random.Generator(np.random.PCG64(int(seed))).integers(0, int(rows.numel()), size=(int(hypotheses), 3), dtype=np.int32)
        cands, n_valid = ops.cloud_ransac(a, b, torch.from_numpy(triples).to(dev), tau, bool(with_scale), float(edge_ratio), int(best),
                                          return_valid=True)
        if n_valid == 0:
            raise ValueError('global_init: RANSAC found no valid hypothesis among %d triples of %d matches (every triangle '
                             'degenerate or its edges unequal beyond edge_ratio = %g)' % (int(hypotheses), int(rows.numel()), float(edge_ratio)))
        reach = np.float32(tau)                                       # the grid's radius is a float32: the next one up where tau rounds down
        reach = float(reach if float(reach) >= tau else np.nextafter(reach, np.float32(np.inf)))
        grid, moved, found = ops.cloud_grid(dst, reach), torch.empty_like(src), []
        for cand in cands:
            if cand['count'] < 0:
                continue
            T = np.vstack([cand['matrix'], [0.0, 0.0, 0.0, 1.0]])
            ops.cloud_transform(src, T, out=moved)
            inside = int(ops.cloud_counts(ops.cloud_nearest(grid, moved)[0], [tau], reach).cpu()[0])
            found.append((inside / float(src.shape[0]), T, cand))
    fitness, T, _ = max(found, key=lambda f: f[0])                    # the first of equals: RANSAC's order
    return {'matrix': T.tolist(), 'fitness': fitness, 'scale': float(np.cbrt(np.linalg.det(T[:3, :3]))),
            'candidates': [{'index': c['index'], 'count': c['count'], 'sum': c['sum'], 'fitness': f} for f, _, c in found],
            'n_recon': int(src.shape[0]), 'n_gt': int(dst.shape[0]), 'n_recon_normals': n_src_normals, 'n_gt_normals': n_dst_normals,
            'n_recon_features': n_src_feat, 'n_gt_features': n_dst_feat, 'n_matches': n_matches, 'n_mutual': n_mutual,
            'mutual_used': mutual_used, 'n_valid_hypotheses': n_valid, 'seed': int(seed), 'with_scale': bool(with_scale),
            'feature_voxel': list(fv), 'feature_radius': list(radius), 'normal_k': int(normal_k), 'feature_k': int(feature_k),
            'tau': tau, 'hypotheses': int(hypotheses), 'mutual': bool(mutual), 'edge_ratio': float(edge_ratio), 'best': int(best)}


def register(recon, gt, init=None, with_scale=False, distances=DEFAULT_DISTANCES, voxel=None, max_iterations=50, min_move=None,
             device=None, icp='point', normals=None, normal_side='source', gt_normals=None, normal_k=16, normal_radius=None,
             global_options=None):
    """Trimmed ICP of `recon` (M,3) onto `gt` (N,3) (host arrays or device tensors, float32) on the device: point-to-point
    (icp='point', the default) or point-to-plane over the reconstruction's normals (icp='plane').

    init: 4x4 starting matrix (None: identity).  with_scale: fit a similarity instead of a rigid motion.  distances: one search
    radius per stage, decreasing.  voxel: both clouds are first reduced by ops.cloud_voxel_downsample with this edge (None: half
    the last distance; 0: the clouds as they are).  Per stage of distance r: ops.cloud_grid(gt, r) once, then per iteration the
    source is moved by the current matrix T, every moved point finds its nearest target within r, the pairs' moments are taken
    between the ORIGINAL source and the target (errors do not compound), and T becomes their closed-form fit; the stage ends when
    the eight corners of the source's bounding box move by at most min_move (None: 1e-3 r; 0: only an exact fixed point stops
    it) or after max_iterations.
    -> dict: matrix (4x4 nested lists: moves the RECONSTRUCTION into the ground truth's frame, `init` included), scale, init,
    with_scale, voxel, n_recon / n_gt (points the fit used), stages [{distance, iterations, pairs, rmse, converged}] (pairs and
    rmse: of the last search, i.e. under the matrix the last fit started from).  A stage with fewer than 3 pairs raises.

    icp='plane' needs normals (M,3), one per row of `recon` in recon's frame (a fused cloud's nx ny nz); they follow their points
    through the down-sampling (a voxel's normal is its first row's); the ground truth needs none.  Per iteration the moments are
    ops.cloud_plane_moments of the ORIGINAL source under the current T about the centre of the target's box, and T becomes
    motion_from_plane_moments(...) T in float64 on the host; stop rule, stages and messages are the same.  The dict then also
    holds icp = 'plane' and, per stage, plane_rmse = sqrt(sum r^2 / pairs) beside rmse; with icp='point' the dict is what it was
    (no icp key), so that what is written from it keeps its bytes.

    normal_side='target' (icp='plane' only) is the classical form of Chen and Medioni over the GROUND TRUTH's normals, for a
    reconstruction that carries none: `normals` is refused, and the moments are ops.cloud_plane_moments_target.  gt_normals: (N,3),
    one per row of `gt` in gt's frame; they follow their points through the down-sampling as the source's do.  None: they are
    estimated once, after the down-sampling, by ops.cloud_grid(gt, normal_radius), ops.cloud_knn(k=normal_k,
    exclude_same_index=True) and ops.cloud_normals(self_counts=True), unoriented -- the step does not see a normal's sign.
    normal_radius None: 4 voxel edges, or twice the last distance when voxel == 0; like normal_k = 16 a default, not a
    measurement.  A target point whose normal is zero (fewer than 3 samples within the radius, or samples along a line) pairs with
    nothing.  The dict then also holds normal_side = 'target', normal_k and normal_radius (both None when gt_normals were given) and
    n_gt_normals, the target points with a usable normal; with normal_side='source' it holds none of them.

    init='global': the start is found from the clouds alone by global_init(recon, gt, with_scale, voxel, **global_options)
    (global_options: its other keyword arguments, e.g. dict(hypotheses=..., seed=..., tau=..., feature_voxel=..., mutual=...)),
    and the loop goes on from its matrix.  The dict then also holds `global`, global_init's dict, and `init` is its matrix; with
    any other init the dict is what it was."""
    import torch
    from .. import ops
    dist = [float(d) for d in distances]
    if not dist or any(not (d > 0.0 and np.isfinite(d)) for d in dist) or any(b >= a for a, b in zip(dist, dist[1:])):
        raise ValueError('distances must be a decreasing list of positive numbers, got %r' % (distances,))
    if voxel is None:
        voxel = dist[-1] / 2.0
    voxel = float(voxel)
    if not (voxel >= 0.0 and np.isfinite(voxel)):
        raise ValueError('voxel must be >= 0, got %r' % voxel)
    if int(max_iterations) < 1:
        raise ValueError('max_iterations must be at least 1')
    if icp not in ('point', 'plane'):
        raise ValueError("icp must be 'point' or 'plane', got %r" % (icp,))
    plane = icp == 'plane'
    if normal_side not in ('source', 'target'):
        raise ValueError("normal_side must be 'source' or 'target', got %r" % (normal_side,))
    target = normal_side == 'target'
    if target and not plane:
        raise ValueError("normal_side='target' is used by icp='plane' only")
    if target and normals is not None:
        raise ValueError("normal_side='target' uses the ground truth's normals (gt_normals=, or estimated): normals= is not used")
    if gt_normals is not None and not target:
        raise ValueError("gt_normals are used by normal_side='target' only")
    if target and gt_normals is None:
        if isinstance(normal_k, bool) or not isinstance(normal_k, (int, np.integer)) or not 2 <= int(normal_k) <= 32:
            raise ValueError('normal_k: expected an integer in 2..32, got %r' % (normal_k,))
        if normal_radius is not None and not (float(normal_radius) > 0.0 and np.isfinite(float(normal_radius))):
            raise ValueError('normal_radius must be positive and finite, got %r' % (normal_radius,))
    if plane and not target and normals is None:
        raise ValueError("icp='plane' needs the reconstruction's normals (normals=, one row per point)")
    if not plane and normals is not None:
        raise ValueError("normals are used by icp='plane' only")
    if isinstance(init, str) and init != 'global':
        raise ValueError("init: a 4x4 matrix, None or 'global', got %r" % (init,))
    if global_options is not None and not isinstance(init, str):
        raise ValueError("global_options are used by init='global' only")
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    found = None
    if isinstance(init, str):
        found = global_init(recon, gt, with_scale=with_scale, voxel=voxel if voxel > 0.0 else dist[-1] / 2.0, device=dev,
                            **(global_options or {}))
        init = found['matrix']
    T0 = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)

    def upload(x):
        if isinstance(x, torch.Tensor):
            return x.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1, 3))).to(dev)

    with torch.cuda.device(dev):
        src, dst = upload(recon), upload(gt)
        nrm = upload(normals) if plane and not target else None
        if nrm is not None and nrm.shape != src.shape:
            raise ValueError('normals: %d rows for %d points' % (nrm.shape[0], src.shape[0]))
        gnrm = upload(gt_normals) if gt_normals is not None else None
        if gnrm is not None and gnrm.shape != dst.shape:
            raise ValueError('gt_normals: %d rows for %d points' % (gnrm.shape[0], dst.shape[0]))
        if voxel > 0.0:
            src, first = ops.cloud_voxel_downsample(src, voxel)
            if nrm is not None:
                nrm = nrm[first.long()].contiguous()
            dst, first = ops.cloud_voxel_downsample(dst, voxel)
            if gnrm is not None:
                gnrm = gnrm[first.long()].contiguous()
        if target and gnrm is None:
            normal_k = int(normal_k)
            normal_radius = float(normal_radius) if normal_radius is not None else (4.0 * voxel if voxel > 0.0 else 2.0 * dist[-1])
            knn = ops.cloud_knn(ops.cloud_grid(dst, normal_radius), dst, normal_k, exclude_same_index=True)[1]
            gnrm = ops.cloud_normals(dst, dst, knn, self_counts=True)
        elif target:
            normal_k = normal_radius = None
        n_gt_normals = int((torch.isfinite(gnrm).all(dim=1) & (gnrm != 0).any(dim=1)).sum().item()) if target else None
        s_lo, s_hi = ops.cloud_bounds(src)
        d_lo, d_hi = ops.cloud_bounds(dst)
        if s_lo is None or d_lo is None:
            raise ValueError('register: a cloud has no finite point')
        corners = box_corners(s_lo, s_hi)
        pivot_src, pivot_dst = (s_lo + s_hi) / 2.0, (d_lo + d_hi) / 2.0
        extent = max(float(np.sqrt(((d_hi - d_lo) ** 2).sum())) / 2.0, np.finfo(np.float64).tiny)
        moved = torch.empty_like(src)
        T, stages = T0.copy(), []
        for k, r in enumerate(dist):
            grid = ops.cloud_grid(dst, r)
            move_tol = 1e-3 * r if min_move is None else float(min_move)
            stage = {'distance': r, 'iterations': 0, 'pairs': 0, 'rmse': None, 'converged': False}
            for _ in range(int(max_iterations)):
                ops.cloud_transform(src, T, out=moved)
                d2, idx = ops.cloud_nearest(grid, moved)
                if target:
                    count, mom = ops.cloud_plane_moments_target(src, T, dst, gnrm, idx, d2, pivot=pivot_dst)
                elif plane:
                    count, mom = ops.cloud_plane_moments(src, nrm, T, dst, idx, d2, pivot=pivot_dst)
                else:
                    count, mom = ops.cloud_pair_moments(src, dst, idx, d2, pivot_src=pivot_src, pivot_dst=pivot_dst)
                if count < 3:
                    raise ValueError('register: %d pairs within %g in stage %d%s' % (
                        count, r, k, ': the initial alignment is too far off for the first distance (give --init_cameras, '
                        '--init_transform or larger --register_distances, or find the start from the clouds alone with '
                        "--register_global / init='global')" if k == 0 and stage['iterations'] == 0 else ''))
                if plane:
                    T_new = motion_from_plane_moments(count, mom, pivot_dst, with_scale, extent) @ T
                else:
                    T_new = similarity_from_moments(count, mom, pivot_src, pivot_dst, with_scale)
                move = corner_move(T, T_new, corners)
                T = T_new
                stage.update(iterations=stage['iterations'] + 1, pairs=count, rmse=float(np.sqrt(mom[-1] / count)))
                if plane:
                    stage['plane_rmse'] = float(np.sqrt(mom[35] / count))
                if move <= move_tol:
                    stage['converged'] = True
                    break
            stages.append(stage)
    result = {'matrix': T.tolist(), 'scale': float(np.cbrt(np.linalg.det(T[:3, :3]))), 'init': T0.tolist(), 'with_scale': bool(with_scale),
              'voxel': voxel, 'n_recon': int(src.shape[0]), 'n_gt': int(dst.shape[0]), 'stages': stages}
    if plane:
        result['icp'] = 'plane'
    if target:
        result.update(normal_side='target', normal_k=normal_k, normal_radius=normal_radius, n_gt_normals=n_gt_normals)
    if found is not None:
        result['global'] = found
    return result
