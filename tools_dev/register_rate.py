"""Registration rate: ops.cloud_transform, cloud_pair_moments and cloud_voxel_downsample alone, one ICP iteration, and a whole
register_cloud.register, on the noisy surfaces of cloud_eval_rate.py with the source moved by a known transform; and the same
iteration on the host, driven by scipy.spatial.cKDTree, as the comparator.

Per size (source x ground truth; default 1M x 1M and 10M x 10M): two noisy unit spheres (the noise is one nearest-neighbour spacing
of the ground truth), the source moved by the inverse of a rotation of 1 degree about (1,2,3) and a translation of two spacings,
R = 5 x 0.6 x the spacing (cloud_eval_rate.py measures 0.6 sqrt(area / n) as the median spacing).  HIP events, medians of --reps
after a warm-up:

    transform_ms    ops.cloud_transform                      24 B per point (12 read, 12 written)
    nearest_ms      ops.cloud_nearest on the moved source (the grid is built once per stage: grid_ms)
    moments_ms      ops.cloud_pair_moments, the 152-byte copy to the host included; 20 B streamed + a 12 B gather per pair
    voxel_ms        ops.cloud_voxel_downsample of the ground truth at voxel = R / 2, its one synchronisation included
    iteration_ms    transform + nearest + moments + the 3x3 fit on the host: one ICP iteration
    register_s      register_cloud.register(source, gt, distances = (4R, 2R, R)) from host arrays to the matrix, wall clock
    host_*          numpy float64 transform, cKDTree(gt) once, tree.query(moved, distance_upper_bound = R, workers = 16), numpy sums:
                    one iteration of the same loop on the host (without scipy the tool says so and times the GPU side only)

--mode plane measures point-to-plane on the same spheres instead (plane_mode): ops.cloud_plane_moments alone (with its 304-byte
copy) against ops.cloud_pair_moments on the same pairs in the same run, one point-to-plane iteration, and register end to end in
both modes with their iteration counts.

    python tools_dev/register_rate.py --out profiles/cloud_register.json
    python tools_dev/register_rate.py --mode plane --out profiles/cloud_register_plane.json
    rocprofv3 --kernel-trace --stats -- python tools_dev/register_rate.py --sizes 10000000x10000000 --skip_host
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
import cloud_register_restated as RR  # noqa: E402
import cloud_restated as CR  # noqa: E402
from colmap_rate import _events_ms  # noqa: E402
from fusion_rate import measured_head  # noqa: E402


def host_iteration(tree, src, gt, T, R):
    """One iteration of the loop on the host -> (T_new, seconds of transform, query, moments + fit)."""
    t0 = time.perf_counter()
    moved = RR.transform(src, T)
    t1 = time.perf_counter()
    dist, idx = tree.query(moved.astype(np.float64), distance_upper_bound=R, workers=16)
    t2 = time.perf_counter()
    keep = np.isfinite(dist)
    T_new = RC.similarity_from_points(src[keep].astype(np.float64), gt[idx[keep]].astype(np.float64), False)
    t3 = time.perf_counter()
    return T_new, t1 - t0, t2 - t1, t3 - t2


def plane_mode(a):
    """--mode plane: ops.cloud_plane_moments alone against ops.cloud_pair_moments (the comparator: the kernel of the parent commit,
    unchanged here) on the SAME pairs in the same run, one point-to-plane iteration, and register_cloud.register end to end in both
    modes with their iteration counts.  The source's normals are the spheres' own (the direction of each point), turned into the
    source's frame.  A sphere leaves the rotation about its centre to the noise alone, so the end-to-end figures say what the loops
    cost here, not how well point-to-plane registers a scene; a refusal of the rank test is recorded as such."""
    import torch
    from atvsnet_amd import ops
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    rows = []
    for size in a.sizes.split(','):
        m, n = (int(v) for v in size.split('x'))
        spacing = float(np.sqrt(4 * np.pi / n))
        gt, src0 = CR.surface(n, 1, noise=spacing), CR.surface(m, 2, noise=spacing)
        Rm = RR.rotation((1, 2, 3), 1.0)
        M = RR.similarity(Rm, (2 * spacing, -spacing, spacing))
        Mi = np.linalg.inv(M)
        src = (src0.astype(np.float64) @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32)
        unit = src0.astype(np.float64) / np.linalg.norm(src0.astype(np.float64), axis=1, keepdims=True)
        nrm = (unit @ Rm).astype(np.float32)                                   # R^T n per row
        R = float(np.float32(5.0 * 0.6 * spacing))
        row = {'source': m, 'ground_truth': n, 'radius': R}
        dS, dN, dG = (torch.from_numpy(x).to(dev) for x in (src, nrm, gt))
        moved = ops.cloud_transform(dS, M)
        grid = ops.cloud_grid(dG, R)
        d2, idx = ops.cloud_nearest(grid, moved)
        lo, hi = ops.cloud_bounds(dG)
        pivot = (lo + hi) / 2.0
        (count, mom), l_ms = _events_ms(lambda: ops.cloud_plane_moments(dS, dN, M, dG, idx, d2, pivot=pivot), a.reps)
        (count_p, _), p_ms = _events_ms(lambda: ops.cloud_pair_moments(dS, dG, idx, d2, pivot_src=pivot, pivot_dst=pivot), a.reps)

        def iteration():
            ops.cloud_transform(dS, M, out=moved)
            dd, ii = ops.cloud_nearest(grid, moved)
            c, mo = ops.cloud_plane_moments(dS, dN, M, dG, ii, dd, pivot=pivot)
            return c, mo
        _, i_ms = _events_ms(iteration, a.reps)
        med = lambda v: float(np.median(v))                                   # noqa: E731
        row.update(plane_moments_ms=med(l_ms), pair_moments_ms=med(p_ms), plane_over_pair=med(l_ms) / med(p_ms),
                   plane_iteration_ms=med(i_ms), plane_moments_ms_all=l_ms, pair_moments_ms_all=p_ms, plane_iteration_ms_all=i_ms,
                   pairs=count, pairs_pair_moments=count_p, plane_rmse=float(np.sqrt(mom[35] / max(count, 1))),
                   plane_bytes_per_pair='32 streamed (src 12, normal 12, idx 4, d2 4) + 12 gathered',
                   pair_bytes_per_pair='20 streamed (src 12, idx 4, d2 4) + 12 gathered',
                   plane_bytes_per_s=(32.0 * m + 12.0 * count) / (med(l_ms) * 1e-3),
                   pair_bytes_per_s=(20.0 * m + 12.0 * count_p) / (med(p_ms) * 1e-3),
                   comparator='ops.cloud_pair_moments (unchanged since the parent commit) on the same pairs, same run')
        print('%d x %d: plane moments %.3f ms (%.2f TB/s), pair moments %.3f ms (%.2f TB/s), ratio %.2f, %d pairs; plane iteration %.2f ms'
              % (m, n, row['plane_moments_ms'], row['plane_bytes_per_s'] / 1e12, row['pair_moments_ms'], row['pair_bytes_per_s'] / 1e12,
                 row['plane_over_pair'], count, row['plane_iteration_ms']), flush=True)
        del dS, dN, dG, moved, grid, d2, idx
        torch.cuda.empty_cache()
        if not a.skip_host:
            dist = (4 * R, 2 * R, R)
            for mode, extra in (('point', {}), ('plane', {'icp': 'plane', 'normals': nrm})):
                try:
                    RC.register(src, gt, distances=dist, **extra)               # warm-up of this size (allocator)
                    times = []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        reg = RC.register(src, gt, distances=dist, **extra)
                        times.append(time.perf_counter() - t0)
                except ValueError as e:
                    row['register_%s_refused' % mode] = str(e)
                    print('  register %s: refused: %s' % (mode, e), flush=True)
                    continue
                T = np.array(reg['matrix'])
                moved_pts = RC.apply(T, src[::max(1, m // 100000)].astype(np.float64))
                row.update({'register_%s_s' % mode: float(np.median(times)), 'register_%s_s_all' % mode: times,
                            'register_%s_stages' % mode: reg['stages'],
                            'register_%s_iterations' % mode: [s['iterations'] for s in reg['stages']],
                            'register_%s_matrix_error' % mode: float(np.abs(T - M).max()),
                            'register_%s_radial_rms' % mode: float(np.sqrt(((np.linalg.norm(moved_pts, axis=1) - 1.0) ** 2).mean()))})
                print('  register %s %.3f s, iterations %s, |T - M| %.2e, radial rms %.2e' % (
                    mode, row['register_%s_s' % mode], row['register_%s_iterations' % mode], row['register_%s_matrix_error' % mode],
                    row['register_%s_radial_rms' % mode]), flush=True)
        rows.append(row)
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'mode': 'plane',
               'results': rows}
    print(json.dumps([{k: v for k, v in r.items() if not k.endswith('_all')} for r in rows]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


def main():
    import torch
    from atvsnet_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('point', 'plane'), default='point',
                    help='plane: cloud_plane_moments against cloud_pair_moments, one point-to-plane iteration, register in both modes')
    ap.add_argument('--sizes', default='1000000x1000000,10000000x10000000', help='source x ground truth, comma-separated')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip_host', action='store_true', help='no host comparator and no whole register (for a kernel trace)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.mode == 'plane':
        return plane_mode(a)
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
        print('scipy is not installed: the GPU side only', flush=True)
    rows = []
    for size in a.sizes.split(','):
        m, n = (int(v) for v in size.split('x'))
        spacing = float(np.sqrt(4 * np.pi / n))
        gt, src0 = CR.surface(n, 1, noise=spacing), CR.surface(m, 2, noise=spacing)
        M = RR.similarity(RR.rotation((1, 2, 3), 1.0), (2 * spacing, -spacing, spacing))
        Mi = np.linalg.inv(M)
        src = (src0.astype(np.float64) @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32)
        R = float(np.float32(5.0 * 0.6 * spacing))
        row = {'source': m, 'ground_truth': n, 'radius': R, 'voxel': R / 2}
        dS, dG = torch.from_numpy(src).to(dev), torch.from_numpy(gt).to(dev)
        moved = torch.empty_like(dS)
        _, t_ms = _events_ms(lambda: ops.cloud_transform(dS, M, out=moved), a.reps)
        grid, g_ms = _events_ms(lambda: ops.cloud_grid(dG, R), a.reps)
        (d2, idx), q_ms = _events_ms(lambda: ops.cloud_nearest(grid, moved), a.reps)
        (count, mom), p_ms = _events_ms(lambda: ops.cloud_pair_moments(dS, dG, idx, d2), a.reps)
        (vox, _), v_ms = _events_ms(lambda: ops.cloud_voxel_downsample(dG, R / 2), a.reps)

        def iteration():
            ops.cloud_transform(dS, M, out=moved)
            dd, ii = ops.cloud_nearest(grid, moved)
            c, mo = ops.cloud_pair_moments(dS, dG, ii, dd)
            return RC.similarity_from_moments(c, mo, None, None, False)
        _, i_ms = _events_ms(iteration, a.reps)
        med = lambda v: float(np.median(v))                                   # noqa: E731
        row.update(transform_ms=med(t_ms), grid_ms=med(g_ms), nearest_ms=med(q_ms), moments_ms=med(p_ms), voxel_ms=med(v_ms),
                   iteration_ms=med(i_ms), transform_ms_all=t_ms, nearest_ms_all=q_ms, moments_ms_all=p_ms, voxel_ms_all=v_ms,
                   iteration_ms_all=i_ms, pairs=count, voxels=int(vox.shape[0]),
                   transform_bytes_per_s=24.0 * m / (med(t_ms) * 1e-3),
                   moments_bytes_per_s=(20.0 * m + 12.0 * count) / (med(p_ms) * 1e-3))
        print('%d x %d: R %.5f; transform %.3f ms (%.2f TB/s), nearest %.2f ms, moments %.3f ms (%.2f TB/s, %d pairs), voxel %.2f ms '
              '(%d voxels), iteration %.2f ms' % (m, n, R, row['transform_ms'], row['transform_bytes_per_s'] / 1e12, row['nearest_ms'],
                                                  row['moments_ms'], row['moments_bytes_per_s'] / 1e12, count, row['voxel_ms'],
                                                  row['voxels'], row['iteration_ms']), flush=True)
        del dS, dG, moved, grid, d2, idx, vox
        torch.cuda.empty_cache()
        if not a.skip_host:
            dist = (4 * R, 2 * R, R)
            RC.register(src, gt, distances=dist)                                # warm-up of this size (allocator)
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                reg = RC.register(src, gt, distances=dist)
                times.append(time.perf_counter() - t0)
            T = np.array(reg['matrix'])
            row.update(register_s=float(np.median(times)), register_s_all=times, register_stages=reg['stages'],
                       register_points=[reg['n_recon'], reg['n_gt']], register_matrix_error=float(np.abs(T - M).max()))
            print('  register %.3f s, stages %s, |T - M| %.2e' % (row['register_s'], [(s['iterations'], s['pairs']) for s in reg['stages']],
                                                                  row['register_matrix_error']), flush=True)
            if cKDTree is not None:
                t0 = time.perf_counter()
                tree = cKDTree(gt.astype(np.float64))
                row['host_tree_build_s'] = time.perf_counter() - t0
                _, ht, hq, hm = host_iteration(tree, src, gt, M, R)
                row.update(host_transform_s=ht, host_query_s=hq, host_moments_fit_s=hm, host_iteration_s=ht + hq + hm,
                           comparator='numpy float64 + scipy.spatial.cKDTree, workers=16')
                print('  host: tree %.1f s; iteration %.2f s = transform %.2f + query %.2f + moments and fit %.2f' %
                      (row['host_tree_build_s'], ht + hq + hm, ht, hq, hm), flush=True)
                del tree
        rows.append(row)
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'results': rows}
    print(json.dumps([{k: v for k, v in r.items() if not k.endswith('_all')} for r in rows]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
