"""Rate of the two ETH3D-style scoring ops (csrc/cloud_visibility.hip, csrc/cloud_register.hip): a noisy unit sphere (the synthetic
scan of tools_dev/cloud_eval_rate.py) with a scanner at its centre, with the numpy restatement on the host as the comparator.

Per size (default 1M and 10M points), after one warm-up, with HIP events around each op, medians of --reps runs:

    render_ms        ops.scan_render of the sphere into the scanner's cube map (6 faces of --cube_size^2, splat 0)
    excess_ms        ops.cloud_scan_excess of a second sample of the sphere (the "reconstruction") at --window
    shares_ms        ops.cloud_voxel_shares of it at --voxel and the six default tolerances (two passes of four)
    points_per_s     points / time, per op
    numpy_*_s        tests/cloud_eth3d_restated.scan_excess / voxel_shares of the first --host_points points on the host, scaled
                     to the size (both are linear in the points); the outputs are compared exactly

The kernels' own times come from a kernel trace of its own run (rocprofv3 --kernel-trace --stats -d DIR -- python
tools_dev/eth3d_eval_rate.py --skip_host); --kernel-stats DIR merges that run's `<DIR>/**/*kernel_stats.csv` into the JSON as
`kernels` (the new kernels' calls, total and average times over the whole traced run).  No rate is a pass / fail bar.  The
expectation to explain a measurement against is arithmetic: per (point, scanner) up to 6 projections of ~40 float64 operations
and two float64 divisions each (3.5 on average: the first face in view ends them), one more division and a square root, plus
(2 window + 1)^2 4-byte gathers; per point and pass of four tolerances at most 4 integer atomics, and one 64-bit compare-and-swap
per probe once.

    python tools_dev/eth3d_eval_rate.py --out profiles/cloud_eth3d.json [--kernel-stats DIR]
"""
import argparse
import csv
import glob
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
import cloud_eth3d_restated as ER  # noqa: E402
import cloud_restated as CR  # noqa: E402
from colmap_rate import _events_ms  # noqa: E402
from fusion_rate import measured_head  # noqa: E402


def kernel_stats(path):
    """The scoring kernels' rows of a rocprofv3 --kernel-trace --stats run under `path`."""
    rows = []
    for f in sorted(glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if any(k in r['Name'] for k in ('scan_excess', 'cloud_share', 'splat_kernel', 'resolve_kernel')):
                    rows.append({'name': r['Name'], 'calls': int(r['Calls']), 'total_ms': float(r['TotalDurationNs']) / 1e6,
                                 'average_us': float(r['AverageNs']) / 1e3})
    return rows


def main():
    import torch
    from atvsnet_amd import ops
    from atvsnet_amd.atvsnet import eval_cloud, eval_eth3d
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000000,10000000', help='points, comma-separated')
    ap.add_argument('--cube_size', type=int, default=1024)
    ap.add_argument('--window', type=int, default=1)
    ap.add_argument('--voxel', type=float, default=0.01)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host_points', type=int, default=200000, help='points the host comparator takes (and the outputs are compared on)')
    ap.add_argument('--skip_host', action='store_true', help='no host comparator (for a kernel trace)')
    ap.add_argument('--kernel-stats', default=None, help='folder of a rocprofv3 --kernel-trace --stats run of this tool')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    tol = list(eval_cloud.DEFAULT_TOLERANCES)
    cams = eval_eth3d.cube_cameras([0.0, 0.0, 0.0], a.cube_size)
    dC = torch.from_numpy(cams).to(dev)
    results = []
    for n in (int(v) for v in a.sizes.split(',')):
        noise = float(np.sqrt(4 * np.pi / n))
        scan, recon = CR.surface(n, 1, noise=noise), CR.surface(n, 2, noise=2 * noise)
        dS, dR = torch.from_numpy(scan).to(dev), torch.from_numpy(recon).to(dev)
        maps, render_ms = _events_ms(lambda: ops.scan_render(dS, dC, a.cube_size, a.cube_size, 0.5, 0), a.reps)
        (excess, scanner), excess_ms = _events_ms(lambda: ops.cloud_scan_excess(dR, dC, maps, 0.5, a.window), a.reps)
        d2, _ = ops.cloud_nearest(ops.cloud_grid(dS, max(tol)), dR)
        org = np.floor(ops.cloud_bounds(dR)[0])
        words, shares_ms = _events_ms(lambda: ops.cloud_voxel_shares(dR, d2, excess, a.voxel, org, tol, 0.0), a.reps)
        row = {'points': n, 'cube_size': a.cube_size, 'window': a.window, 'voxel': a.voxel, 'tolerances': tol,
               'render_ms': float(np.median(render_ms)), 'render_ms_all': render_ms,
               'excess_ms': float(np.median(excess_ms)), 'excess_ms_all': excess_ms,
               'shares_ms': float(np.median(shares_ms)), 'shares_ms_all': shares_ms,
               'excess_points_per_s': n / (float(np.median(excess_ms)) * 1e-3),
               'shares_points_per_s': n / (float(np.median(shares_ms)) * 1e-3),
               'covered_share': float((maps > 0).double().mean()), 'observed_share': float((scanner >= 0).double().mean()),
               'voxels': int(words[0, 1])}
        if not a.skip_host:
            k = min(a.host_points, n)
            host_maps = maps.cpu().numpy()
            t0 = time.perf_counter()
            want_e, want_s = ER.scan_excess(recon[:k], cams, host_maps, 0.5, a.window)
            t1 = time.perf_counter()
            host_d2 = d2[:k].cpu().numpy()
            want_w = ER.voxel_shares(recon[:k], host_d2, want_e, a.voxel, org, tol, 0.0)
            t2 = time.perf_counter()
            got_w = ops.cloud_voxel_shares(dR[:k], d2[:k].contiguous(), excess[:k].contiguous(), a.voxel, org, tol, 0.0).cpu().tolist()
            same = bool(np.array_equal(excess[:k].cpu().numpy().view(np.uint32), want_e.view(np.uint32)) and
                        np.array_equal(scanner[:k].cpu().numpy(), want_s) and got_w == want_w)
            row.update(numpy_excess_s=(t1 - t0) * n / k, numpy_shares_s=(t2 - t1) * n / k, numpy_points_measured=k,
                       comparator='numpy restatement (float64; np.unique and Python integers), scaled from %d points' % k,
                       agrees_with_comparator=same)
            if not same:
                raise SystemExit('the GPU result disagrees with the restatement')
        print(json.dumps({k: v for k, v in row.items() if not k.endswith('_all')}), flush=True)
        results.append(row)
        del dS, dR, maps, excess, scanner, d2, words
        torch.cuda.empty_cache()
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'results': results}
    if a.kernel_stats:
        summary['kernels'] = kernel_stats(a.kernel_stats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
