"""PCA-normal rate (csrc/cloud_normals.hip) beside the k-nearest-neighbour search that feeds it, a host k-d tree + batched
eigen-decomposition as the comparator, and the three registrations of DESIGN.md section 12.1a at size.

Per size (default 1M and 10M points) a noisy unit sphere is drawn as tools_dev/knn_rate.py draws it, searched in itself with
R = 5 x the median nearest-neighbour spacing, and for k in {8, 16, 32}, after one warm-up, with HIP events around the calls, medians
of --reps runs:

    grid_ms      ops.cloud_grid
    knn_ms       ops.cloud_knn(exclude_same_index=True) on that grid: the counting sort of the queries + the search kernel
    normals_ms   ops.cloud_normals(self_counts=True) over its idx: one launch
    host_s       scipy.spatial.cKDTree.query(k=k+1, distance_upper_bound=R, workers=16) + numpy.linalg.eigh over the (n,3,3)
                 covariances (float64, numpy sums), on the host, over the first --host_points points' rows; the share of those rows
                 whose normal agrees with the kernel's to 1e-5 (sine of the angle, rows with a relative eigen-gap above 1e-3)

and, with --register_points (default 1M x 1M), register_cloud.register on the comparison pair of tests/cloud_plane_restated.py
scaled to that size, wall time (the median and every one of --reps calls after one warm-up call of that way) and iterations, three ways: icp='point', icp='plane' with the source's analytic normals,
icp='plane' normal_side='target' with the target's estimated (k = 16).  The kernel is never compared with itself.

    python tools_dev/cloud_normals_rate.py --out profiles/cloud_normals.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import atvsnet_amd  # noqa: E402,F401
from atvsnet_amd.atvsnet import register_cloud as RC  # noqa: E402
import cloud_plane_restated as PR  # noqa: E402
import cloud_restated as CR  # noqa: E402
from colmap_rate import _events_ms  # noqa: E402
from fusion_rate import measured_head  # noqa: E402


def host_normals(tree, P, rows, k, R):
    """-> (normals (rows,3) float64 unoriented, gap (rows,), seconds): cKDTree + batched eigh over the first `rows` points."""
    t0 = time.perf_counter()
    dist, ti = tree.query(P[:rows].astype(np.float64), k=k + 1, distance_upper_bound=R, workers=16)
    ok = np.isfinite(dist)                                               # the query itself is its own first hit: it counts
    d = np.where(ok[:, :, None], P[np.where(ok, ti, 0)].astype(np.float64) - P[:rows, None, :].astype(np.float64), 0.0)
    c = ok.sum(axis=1).astype(np.float64)
    s = d.sum(axis=1)
    C = np.einsum('nka,nkb->nab', d, d) - s[:, :, None] * s[:, None, :] / c[:, None, None]
    w, V = np.linalg.eigh(C)
    seconds = time.perf_counter() - t0
    with np.errstate(divide='ignore', invalid='ignore'):
        return V[:, :, 0], (w[:, 1] - w[:, 0]) / w[:, 2], seconds


def main():
    import torch
    from atvsnet_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000000,10000000', help='points, comma-separated')
    ap.add_argument('--ks', default='8,16,32')
    ap.add_argument('--radius', type=float, default=5.0, help='in multiples of the median nearest-neighbour spacing')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host_points', type=int, default=1000000, help='rows the host comparator answers (0: no comparator)')
    ap.add_argument('--register_points', type=int, default=1000000, help='points per cloud of the three registrations (0: none)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cKDTree = None
    if a.host_points:
        from scipy.spatial import cKDTree
    rows = []
    for n in (int(v) for v in a.sizes.split(',')):
        area_spacing = float(np.sqrt(4 * np.pi / n))
        P = CR.surface(n, 1, noise=area_spacing)
        dP = torch.from_numpy(P).to(dev)
        d2 = ops.cloud_knn(ops.cloud_grid(dP, 4.0 * area_spacing), dP, 1, exclude_same_index=True)[0][:, 0]
        spacing = float(torch.sqrt(d2[torch.isfinite(d2)].double()).median())
        R = float(np.float32(a.radius * spacing))
        tree = cKDTree(P.astype(np.float64)) if cKDTree is not None else None
        grid, g_ms = _events_ms(lambda: ops.cloud_grid(dP, R), a.reps)
        for k in (int(v) for v in a.ks.split(',')):
            (_, idx), k_ms = _events_ms(lambda: ops.cloud_knn(grid, dP, k, exclude_same_index=True), a.reps)
            nrm, n_ms = _events_ms(lambda: ops.cloud_normals(dP, dP, idx, self_counts=True), a.reps)
            row = {'points': n, 'k': k, 'spacing': spacing, 'radius': R, 'grid_ms': float(np.median(g_ms)), 'knn_ms': float(np.median(k_ms)),
                   'normals_ms': float(np.median(n_ms)), 'normals_ms_all': n_ms, 'knn_ms_all': k_ms,
                   'gather_bytes_per_row': 12 * k + 4 * k + 12 + 12,
                   'zero_normals_share': float((~(nrm != 0).any(dim=1)).double().mean())}
            if tree is not None:
                sub = min(a.host_points, n)
                want, gap, seconds = host_normals(tree, P, sub, k, R)
                got = nrm[:sub].cpu().numpy().astype(np.float64)
                sure = got.any(axis=1) & (gap > 1e-3)
                sin = np.linalg.norm(np.cross(got[sure], want[sure]), axis=1)
                row.update(host_rows=sub, host_s=seconds, comparator='scipy.spatial.cKDTree.query(k=k+1, workers=16) + numpy.linalg.eigh',
                           host_rows_compared=int(sure.sum()), host_agree_share=float((sin <= 1e-5).mean()) if sure.any() else None)
            print(json.dumps({key: v for key, v in row.items() if not key.endswith('_all')}), flush=True)
            rows.append(row)
            del idx, nrm
        del grid, dP, tree
        torch.cuda.empty_cache()
    registrations = []
    if a.register_points:
        gt, src, nrm, M = PR.sampled_pair(a.register_points, a.register_points, 21, 22)
        common = dict(distances=PR.STAGES, voxel=0, max_iterations=100, min_move=PR.MIN_MOVE)
        ways = (('point', {}), ('plane, source normals (analytic)', dict(icp='plane', normals=nrm)),
                ('plane, target normals (estimated, k = 16, radius 0.02)', dict(icp='plane', normal_side='target', normal_radius=0.02)))
        for name, extra in ways:
            reg = RC.register(src, gt, **dict(common, **extra))          # the warm-up of this way: its kernels' first launches, the allocator
            times = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                again = RC.register(src, gt, **dict(common, **extra))
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                assert again == reg                                      # the same input: the same dict
            registrations.append({'way': name, 'points': a.register_points, 'seconds': float(np.median(times)), 'seconds_all': times,
                                  'iterations': [s['iterations'] for s in reg['stages']],
                                  'corner_error': PR.corner_error(np.array(reg['matrix']), M, src)})
            print(json.dumps(registrations[-1]), flush=True)
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'results': rows,
               'registrations': registrations}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
