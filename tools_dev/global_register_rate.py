"""Global registration rate: ops.cloud_fpfh, ops.cloud_feature_nearest and ops.cloud_ransac alone, and a whole
register_cloud.global_init, on the asymmetric room of tests/cloud_register_restated.py turned by 150 degrees and moved several room
sizes away; beside them the numpy restatement of the same steps (tests/cloud_global_restated.py), which is the comparator.

Per size (raw points per cloud; default 20000 and 200000): the room with noise of a fifth of its mean spacing, the source the same
cloud under a known motion.  The kernels alone run at a DENSE feature voxel, twice the mean spacing (about a quarter of the points
stay: the kernels' rates at 5k and 50k rows); such a voxel is a 75th and a 240th of the room's diagonal, and five of them span
nothing but flat wall, so global_init at it is timed and its result recorded as it is (global_init_dense_*), while global_init_s
runs at a 64th of the diagonal, the rule register_cloud.global_init applies with_scale.  HIP events, medians of --reps after a
warm-up:

    fpfh_ms             ops.cloud_fpfh of the down-sampled target over 32 neighbours (two launches)
    feature_nearest_ms  ops.cloud_feature_nearest, every source descriptor against every target descriptor
    ransac_ms           ops.cloud_ransac, --hypotheses triples over the matches, the 15 x best words' copy included
    global_init_s       register_cloud.global_init from host arrays to the matrix, wall clock, and how far its matrix is from the
                        true motion at the corners of the source's box (corner_error; fitness; valid hypotheses)
    host_*              the restatement's fpfh, feature_nearest, ransac and global_init, one call each (--skip_host: none; sizes
                        above --host_limit raw points are skipped: the restated matching is quadratic in memory-bound numpy)

    python tools_dev/global_register_rate.py --out profiles/cloud_global_register.json
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
import cloud_global_restated as GR  # noqa: E402
import cloud_register_restated as RR  # noqa: E402
from colmap_rate import _events_ms  # noqa: E402
from fusion_rate import measured_head  # noqa: E402


def _clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def main():
    import torch
    from atvsnet_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='20000,200000', help='raw points per cloud, comma-separated')
    ap.add_argument('--hypotheses', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--skip_host', action='store_true', help='no restatement beside the kernels')
    ap.add_argument('--host_limit', type=int, default=50000, help='largest size the restatement is timed on')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    med = lambda v: float(np.median(v))                                       # noqa: E731
    rows = []
    for n in (int(v) for v in a.sizes.split(',')):
        spacing = float(np.sqrt(5.35 / n))                                    # the room's area is 5.35
        gt = RR.shape(n, 1, 0.2 * spacing).astype(np.float32)
        M = RR.similarity(RR.rotation((1, -2, 0.5), 150.0), (7.0, -5.0, 9.0), 1.0, gt.astype(np.float64).mean(axis=0))
        Mi = np.linalg.inv(M)
        src = (gt.astype(np.float64) @ Mi[:3, :3].T + Mi[:3, 3]).astype(np.float32)
        fv = 2.0 * spacing
        row = {'points': n, 'dense_feature_voxel': fv, 'feature_voxel': GR.bounds_diagonal(gt) / 64.0, 'hypotheses': a.hypotheses}
        # the three kernels alone, on what global_init feeds them
        clouds = []
        for cloud in (src, gt):
            down = ops.cloud_voxel_downsample(torch.from_numpy(cloud).to(dev), fv)[0].contiguous()
            knn = ops.cloud_knn(ops.cloud_grid(down, 5.0 * fv), down, 32, exclude_same_index=True)[1]
            nrm = ops.cloud_normals(down, down, knn[:, :16].contiguous(), self_counts=True)
            clouds.append((down, knn, nrm))
        (dS, kS, nS), (dG, kG, nG) = clouds
        fG, f_ms = _events_ms(lambda: ops.cloud_fpfh(dG, kG, nG), a.reps)
        fS = ops.cloud_fpfh(dS, kS, nS)
        (_, fwd), m_ms = _events_ms(lambda: ops.cloud_feature_nearest(fG, fS), a.reps)
        keep = torch.nonzero(fwd >= 0).reshape(-1)
        pa, pb = dS[keep].contiguous(), dG[fwd.long()[keep]].contiguous()
        triples = np.random.Generator(np.random.PCG64(0)).integers(0, int(keep.numel()), size=(a.hypotheses, 3), dtype=np.int32)
        dT = torch.from_numpy(triples).to(dev)
        best, r_ms = _events_ms(lambda: ops.cloud_ransac(pa, pb, dT, 1.5 * fv, False), a.reps)
        row.update(feature_points=[int(dS.shape[0]), int(dG.shape[0])], matches=int(keep.numel()), fpfh_ms=med(f_ms),
                   feature_nearest_ms=med(m_ms), ransac_ms=med(r_ms), fpfh_ms_all=f_ms, feature_nearest_ms_all=m_ms, ransac_ms_all=r_ms,
                   ransac_best_count=best[0]['count'])
        print('%d points: %d x %d feature points, %d matches; fpfh %.3f ms, feature_nearest %.3f ms, ransac %.3f ms (best count %d)' % (
            n, dS.shape[0], dG.shape[0], keep.numel(), row['fpfh_ms'], row['feature_nearest_ms'], row['ransac_ms'], best[0]['count']), flush=True)
        for name, voxel in (('global_init', row['feature_voxel']), ('global_init_dense', fv)):
            options = dict(feature_voxel=voxel, hypotheses=a.hypotheses)
            RC.global_init(src, gt, **options)                                # warm-up of this size (allocator)
            times = []
            for _ in range(a.reps):
                found, s = _clock(lambda: RC.global_init(src, gt, **options))
                times.append(s)
            row.update({name + '_s': med(times), name + '_s_all': times, name + '_fitness': found['fitness'],
                        name + '_valid_hypotheses': found['n_valid_hypotheses'], name + '_points': [found['n_recon'], found['n_gt']],
                        name + '_corner_error': GR.corner_error(np.array(found['matrix']), M, src)})
            print('  %s (voxel %.4f, %d x %d points) %.3f s, fitness %.3f, %d valid hypotheses, %.4f from the true motion' % (
                name, voxel, found['n_recon'], found['n_gt'], row[name + '_s'], found['fitness'], found['n_valid_hypotheses'],
                row[name + '_corner_error']), flush=True)
        if not a.skip_host and n <= a.host_limit:
            hG, hk, hn = (t.cpu().numpy() for t in (dG, kG, nG))
            (_, _), row['host_fpfh_s'] = _clock(lambda: GR.fpfh(hG, hk, hn))
            (_, _), row['host_feature_nearest_s'] = _clock(lambda: GR.feature_nearest(fG.cpu().numpy(), fS.cpu().numpy()))
            _, row['host_ransac_s'] = _clock(lambda: GR.ransac(pa.cpu().numpy(), pb.cpu().numpy(), triples, 1.5 * fv, False))
            host, row['host_global_init_s'] = _clock(lambda: GR.global_init(src, gt, hypotheses=a.hypotheses,
                                                                            feature_voxel=row['feature_voxel']))
            row.update(host_corner_error=GR.corner_error(host['matrix'], M, src), comparator='the numpy restatement, one call each')
            print('  host: fpfh %.2f s, feature_nearest %.2f s, ransac %.2f s, global_init %.2f s (%.4f from the true motion)' % (
                row['host_fpfh_s'], row['host_feature_nearest_s'], row['host_ransac_s'], row['host_global_init_s'],
                row['host_corner_error']), flush=True)
        rows.append(row)
        del clouds, dS, dG, fG, fS, pa, pb, dT
        torch.cuda.empty_cache()
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'results': rows}
    print(json.dumps([{k: v for k, v in r.items() if not k.endswith('_all')} for r in rows]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
