"""Point-cloud scoring rate: grid build, nearest-neighbour query and tolerance counts (csrc/cloud.hip) on a synthetic scanned
surface, the whole eval_cloud.evaluate call, and a host k-d tree on the same arrays as the comparator.

Per size (queries x reference points; default 1M x 1M, 2M x 10M, 10M x 10M) two noisy unit spheres are drawn (the noise is one
nearest-neighbour spacing of the reference cloud), R = 5 x the median nearest-neighbour spacing of the reference cloud, and after
one warm-up, with HIP events around the calls, medians of --reps runs:

    grid_ms      ops.cloud_grid (bounding box, cell parameters, counting sort of the reference cloud)
    nearest_ms   ops.cloud_nearest (counting sort of the queries by the grid's cells + the query kernel)
    counts_ms    ops.cloud_counts, six tolerances
    evaluate_s   eval_cloud.evaluate from host arrays to the result dict: uploads, both directions, downloads, host statistics
    kdtree_*_s   scipy.spatial.cKDTree(reference) and .query(queries, distance_upper_bound=R, workers=16), float64, on the host
                 (without scipy: the chunked numpy restatement on a 100k x 100k subset, named so)

and the bytes the query must move: every query reads the records (16 B) of the 27 cells around it -- `bytes_no_reuse` -- or, were
every record read once per query CELL, `bytes_cell_reuse`; both from the cell occupancy counted on the host.  The query kernel's own
time is in the kernel trace (rocprofv3 --kernel-trace --stats -- python tools_dev/cloud_eval_rate.py --sizes 10000000x10000000
--skip_host), not here: nearest_ms includes the queries' sort.  The GPU results are checked against the tree (found / not found
outside a 1e-6 band around R, and the float32 d2 of the tree's neighbour not below the reported one).

    python tools_dev/cloud_eval_rate.py --out profiles/cloud_eval.json
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
from atvsnet_amd.atvsnet import eval_cloud  # noqa: E402
import cloud_restated as CR  # noqa: E402
from colmap_rate import _events_ms  # noqa: E402
from fusion_rate import measured_head  # noqa: E402

TOLERANCE_SHARES = (0.1, 0.2, 0.4, 0.6, 0.8, 1.0)         # of R


def cell_traffic(Q, P, R):
    """Bytes of reference records the query reads: per query the 27 cells around it; and once per distinct query cell."""
    h = float(np.float32(R)) * (1.0 + 2.0 ** -20)
    lo = P.min(axis=0).astype(np.float64)
    dims = np.floor((P.max(axis=0).astype(np.float64) - lo) / h).astype(np.int64) + 1
    cp = np.floor((P.astype(np.float64) - lo) / h).astype(np.int64)
    occ = np.bincount((cp[:, 2] * dims[1] + cp[:, 1]) * dims[0] + cp[:, 0], minlength=int(dims.prod()))
    vol = occ.reshape(dims[2], dims[1], dims[0])
    pad = np.pad(vol, 1)
    around = sum(pad[1 + dz:1 + dz + dims[2], 1 + dy:1 + dy + dims[1], 1 + dx:1 + dx + dims[0]]
                 for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)).reshape(-1)
    t = np.floor((Q.astype(np.float64) - lo) / h)
    near = ((t >= -1) & (t <= dims)).all(axis=1)
    cq = np.clip(t[near].astype(np.int64), 0, dims - 1)
    nq = np.bincount((cq[:, 2] * dims[1] + cq[:, 1]) * dims[0] + cq[:, 0], minlength=int(dims.prod()))
    return {'cells': int(dims.prod()), 'occupied_cells': int((occ > 0).sum()), 'mean_occupancy_of_occupied_cells': float(occ[occ > 0].mean()),
            'candidates_per_query': float((nq * around).sum() / max(1, len(Q))),
            'bytes_no_reuse': int((nq * around).sum()) * 16, 'bytes_cell_reuse': int(around[nq > 0].sum()) * 16}


def main():
    import torch
    from atvsnet_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000000x1000000,2000000x10000000,10000000x10000000', help='queries x reference, comma-separated')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip_host', action='store_true', help='no host comparator, no evaluate, no traffic count (for a kernel trace)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    rows = []
    for size in a.sizes.split(','):
        m, n = (int(v) for v in size.split('x'))
        spacing = float(np.sqrt(4 * np.pi / n))                     # of n points on a unit sphere
        P, Q = CR.surface(n, 1, noise=spacing), CR.surface(m, 2, noise=spacing)
        row = {'queries': m, 'reference': n}
        tree = None
        if cKDTree is not None and not a.skip_host:
            t0 = time.perf_counter()
            tree = cKDTree(P.astype(np.float64))
            row['kdtree_build_s'] = time.perf_counter() - t0
            nn = tree.query(P[:100000].astype(np.float64), k=2, workers=16)[0][:, 1]
            R = float(np.float32(5.0 * np.median(nn)))
        else:
            R = float(np.float32(5.0 * 0.6 * spacing))              # (a k-d tree measures a median spacing of about 0.6 sqrt(area / n))
        row['radius'] = R
        tol = [s * R for s in TOLERANCE_SHARES]
        dP, dQ = torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev)
        grid, g_ms = _events_ms(lambda: ops.cloud_grid(dP, R), a.reps)
        (d2, idx), q_ms = _events_ms(lambda: ops.cloud_nearest(grid, dQ), a.reps)
        cnt, c_ms = _events_ms(lambda: ops.cloud_counts(d2, tol, R), a.reps)
        row.update(grid_ms=float(np.median(g_ms)), nearest_ms=float(np.median(q_ms)), counts_ms=float(np.median(c_ms)),
                   grid_ms_all=g_ms, nearest_ms_all=q_ms, counts_ms_all=c_ms, grid_bytes=grid.nbytes,
                   found_share=float((idx >= 0).float().mean()))
        print('%d x %d: R %.5f, grid %.2f ms, nearest %.2f ms, counts %.3f ms, found %.3f' %
              (m, n, R, row['grid_ms'], row['nearest_ms'], row['counts_ms'], row['found_share']), flush=True)
        if not a.skip_host:
            eval_cloud.evaluate(Q, P, tol, R)                          # warm-up of this size (allocator)
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                eval_cloud.evaluate(Q, P, tol, R)
                times.append(time.perf_counter() - t0)
            row.update(evaluate_s=float(np.median(times)), evaluate_s_all=times)
            row.update(cell_traffic(Q, P, R))
            print('  evaluate %.3f s; %.0f candidates per query, %.2f GB without reuse, %.3f GB with cell reuse' %
                  (row['evaluate_s'], row['candidates_per_query'], row['bytes_no_reuse'] / 1e9, row['bytes_cell_reuse'] / 1e9), flush=True)
            hd2, hidx = d2.cpu().numpy(), idx.cpu().numpy()
            if tree is not None:
                t0 = time.perf_counter()
                dist, ti = tree.query(Q.astype(np.float64), distance_upper_bound=R, workers=16)
                row['kdtree_query_s'] = time.perf_counter() - t0
                row['comparator'] = 'scipy.spatial.cKDTree, float64, workers=16'
                found, tfound = hidx >= 0, np.isfinite(dist)
                band = np.abs(dist - R) <= 1e-6 * R
                both = found & tfound
                same = bool(np.array_equal(found[~band], tfound[~band]) and (hd2[both] <= CR.d2_pairs(Q[both], P[ti[both]])).all())
                print('  k-d tree build %.1f s, query %.1f s' % (row['kdtree_build_s'], row['kdtree_query_s']), flush=True)
            else:
                k = min(100000, m, n)
                t0 = time.perf_counter()
                want = CR.nearest(Q[:k], P[:k], R)
                row['numpy_restatement_100k_x_100k_s'] = time.perf_counter() - t0
                row['comparator'] = 'chunked numpy restatement on a %d x %d subset' % (k, k)
                sub = ops.cloud_nearest(ops.cloud_grid(dP[:k].contiguous(), R), dQ[:k].contiguous())
                same = bool(np.array_equal(sub[0].cpu().numpy(), want[0]) and np.array_equal(sub[1].cpu().numpy(), want[1]))
            row['agrees_with_comparator'] = same
            if not same:
                raise SystemExit('the GPU result disagrees with the comparator')
        rows.append(row)
        del dP, dQ, grid, d2, idx, tree
        torch.cuda.empty_cache()
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps,
               'tolerances_as_shares_of_R': TOLERANCE_SHARES, 'results': rows}
    print(json.dumps([{k: v for k, v in r.items() if not k.endswith('_all')} for r in rows]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
