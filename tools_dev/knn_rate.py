"""k-nearest-neighbour search rate (csrc/cloud_knn.hip) on a synthetic scanned surface searched in itself, the whole
clean_cloud.clean call, and a host k-d tree on the same array as the comparator.

Per size (default 1M and 10M points) a noisy unit sphere is drawn as tools_dev/cloud_eval_rate.py draws it (the noise is one
nearest-neighbour spacing), and for R in {3, 5} x the median nearest-neighbour spacing and k in {8, 16, 32}, after one warm-up, with
HIP events around the calls, medians of --reps runs:

    grid_ms      ops.cloud_grid
    knn_ms       ops.cloud_knn(exclude_same_index=True): the counting sort of the queries + the search kernel
    nearest_ms   ops.cloud_nearest on the same grid and queries (the k = 1 search this one is measured against)
    count_ms     ops.cloud_radius_count
    clean_s      clean_cloud.clean(sor=(k, 2.0, R)) from host arrays to host arrays (k = 8 only)
    kdtree_query_s   scipy.spatial.cKDTree.query(k=k+1, distance_upper_bound=R, workers=16), float64, on the host; without scipy the
                 numpy restatement (tests/cloud_knn_restated.py) on a 20k subset, named so

with the candidates per query (the records of the 27 cells, counted on the host) and the share of rows with k neighbours.  The
kernels' own times are in the kernel trace (rocprofv3 --kernel-trace --stats -- python tools_dev/knn_rate.py --sizes 10000000
--skip_host), not here: knn_ms includes the queries' sort.

    python tools_dev/knn_rate.py --out profiles/cloud_knn.json
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
from atvsnet_amd.atvsnet import clean_cloud  # noqa: E402
import cloud_knn_restated as KR  # noqa: E402
import cloud_restated as CR  # noqa: E402
from cloud_eval_rate import cell_traffic  # noqa: E402
from colmap_rate import _events_ms  # noqa: E402
from fusion_rate import measured_head  # noqa: E402


def main():
    import torch
    from atvsnet_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000000,10000000', help='points, comma-separated')
    ap.add_argument('--ks', default='8,16,32')
    ap.add_argument('--radii', default='3,5', help='multiples of the median nearest-neighbour spacing')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip_host', action='store_true', help='no host comparator, no clean, no candidate count (for a kernel trace)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    ks = [int(k) for k in a.ks.split(',')]
    rows = []
    for n in (int(v) for v in a.sizes.split(',')):
        area_spacing = float(np.sqrt(4 * np.pi / n))
        P = CR.surface(n, 1, noise=area_spacing)
        dP = torch.from_numpy(P).to(dev)
        # the median nearest-neighbour spacing, by the kernels themselves on a generous radius
        d2 = ops.cloud_knn(ops.cloud_grid(dP, 4.0 * area_spacing), dP, 1, exclude_same_index=True)[0][:, 0]
        spacing = float(torch.sqrt(d2[torch.isfinite(d2)].double()).median())
        tree = None
        if cKDTree is not None and not a.skip_host:
            t0 = time.perf_counter()
            tree = cKDTree(P.astype(np.float64))
            build_s = time.perf_counter() - t0
        for mult in (float(v) for v in a.radii.split(',')):
            R = float(np.float32(mult * spacing))
            grid, g_ms = _events_ms(lambda: ops.cloud_grid(dP, R), a.reps)
            _, n_ms = _events_ms(lambda: ops.cloud_nearest(grid, dP), a.reps)
            cnt, c_ms = _events_ms(lambda: ops.cloud_radius_count(grid, dP, exclude_same_index=True), a.reps)
            base = {'points': n, 'spacing': spacing, 'radius_in_spacings': mult, 'radius': R, 'grid_ms': float(np.median(g_ms)),
                    'nearest_ms': float(np.median(n_ms)), 'count_ms': float(np.median(c_ms)),
                    'neighbours_in_radius_mean': float(cnt.double().mean())}
            if not a.skip_host:
                base['candidates_per_query'] = cell_traffic(P, P, R)['candidates_per_query']
            for k in ks:
                (kd2, kidx), k_ms = _events_ms(lambda: ops.cloud_knn(grid, dP, k, exclude_same_index=True), a.reps)
                row = dict(base, k=k, knn_ms=float(np.median(k_ms)), knn_ms_all=k_ms,
                           full_rows_share=float((kidx[:, k - 1] >= 0).double().mean()))
                print('%d points, R = %g spacings, k = %d: grid %.2f ms, knn %.2f ms (nearest %.2f ms, count %.2f ms), full rows %.3f'
                      % (n, mult, k, row['grid_ms'], row['knn_ms'], row['nearest_ms'], row['count_ms'], row['full_rows_share']), flush=True)
                if not a.skip_host:
                    hidx = kidx.cpu().numpy()
                    if tree is not None:
                        t0 = time.perf_counter()
                        dist, ti = tree.query(P.astype(np.float64), k=k + 1, distance_upper_bound=R, workers=16)
                        row.update(kdtree_build_s=build_s, kdtree_query_s=time.perf_counter() - t0,
                                   comparator='scipy.spatial.cKDTree.query(k=k+1), float64, workers=16')
                        # the tree counts the query itself: k + 1 hits there are k neighbours here (outside a band around R)
                        band = (np.abs(dist - R) <= 1e-6 * R).any(axis=1)
                        same = bool(np.array_equal((np.isfinite(dist).sum(axis=1) - 1)[~band], (hidx >= 0).sum(axis=1)[~band]))
                    else:
                        sub = min(20000, n)
                        t0 = time.perf_counter()
                        want = KR.knn(P[:sub], P[:sub], R, k, True)
                        row.update(numpy_restatement_20k_s=time.perf_counter() - t0,
                                   comparator='numpy restatement on a %d-point subset' % sub)
                        head = dP[:sub].contiguous()
                        got = ops.cloud_knn(ops.cloud_grid(head, R), head, k, exclude_same_index=True)
                        same = bool(np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]))
                    row['agrees_with_comparator'] = same
                    if not same:
                        raise SystemExit('the GPU result disagrees with the comparator')
                    if k == ks[0]:
                        clean_cloud.clean(P, None, sor=(k, 2.0, R))              # warm-up of this size (allocator)
                        times = []
                        for _ in range(a.reps):
                            t0 = time.perf_counter()
                            out = clean_cloud.clean(P, None, sor=(k, 2.0, R))
                            times.append(time.perf_counter() - t0)
                        row.update(clean_s=float(np.median(times)), clean_rows_out=int(out[2]['n_out']))
                        print('  clean(sor=(%d, 2.0, R)) %.3f s, %d of %d rows stay' % (k, row['clean_s'], row['clean_rows_out'], n), flush=True)
                rows.append(row)
                del kd2, kidx
            del grid, cnt
        del dP, tree
        torch.cuda.empty_cache()
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'results': rows}
    print(json.dumps([{k: v for k, v in r.items() if not k.endswith('_all')} for r in rows]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
