"""Scan rendering rate (csrc/scan_render.hip): a noisy unit sphere (the synthetic scan of tools_dev/cloud_eval_rate.py) rendered
into a ring of cameras around it, with the numpy restatement on the host, one camera at a time, as the comparator.

Per size (default 1M and 10M points), ring (default 16 and 64 cameras of 228 x 120) and splat (default 0 and 2), after one warm-up,
with HIP events around ops.scan_render (memset + splat + resolve; the scratch allocation is the caching allocator's), medians of
--reps runs:

    render_ms        ops.scan_render
    pairs_per_s      points x cameras / render time
    in_view_share    the share of (camera, point) pairs that land in an image (from the restatement; with it only)
    numpy_s          tests/scan_render_restated.scan_render of the same inputs on the host (--host_cams cameras of the ring,
                     scaled to the ring: one camera at a time, so it is linear in the cameras); the output is compared bit for bit

The kernels' own times are in a kernel trace of its own run (rocprofv3 --kernel-trace --stats -- python tools_dev/render_rate.py
--skip_host), not here.  No rate is a pass / fail bar.  The expectation to explain a measurement against is arithmetic: about 40
float64 operations and two float64 divisions per pair, plus (2 splat + 1)^2 + 1 atomics per pair in view (1 at splat 0).

    python tools_dev/render_rate.py --out profiles/scan_render.json
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
import cloud_restated as CR  # noqa: E402
import scan_render_restated as SR  # noqa: E402
from colmap_rate import _events_ms  # noqa: E402
from fusion_rate import measured_head  # noqa: E402


def main():
    import torch
    from atvsnet_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1000000,10000000', help='points, comma-separated')
    ap.add_argument('--cams', default='16,64', help='cameras on the ring, comma-separated')
    ap.add_argument('--splats', default='0,2')
    ap.add_argument('--rows', type=int, default=120)
    ap.add_argument('--cols', type=int, default=228)
    ap.add_argument('--occlusion_tol', type=float, default=0.05)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host_cams', type=int, default=2, help='cameras the host comparator renders (and the output is compared on)')
    ap.add_argument('--skip_host', action='store_true', help='no host comparator (for a kernel trace)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    results = []
    for n in (int(v) for v in a.sizes.split(',')):
        P = CR.surface(n, 1, noise=float(np.sqrt(4 * np.pi / n)))
        dP = torch.from_numpy(P).to(dev)
        for n_cams in (int(v) for v in a.cams.split(',')):
            cams = SR.ring_cameras(n_cams, a.rows, a.cols, radius=3.0)
            dC = torch.from_numpy(cams).to(dev)
            for splat in (int(v) for v in a.splats.split(',')):
                tol = a.occlusion_tol if splat else 0.0
                depth, ms = _events_ms(lambda: ops.scan_render(dP, dC, a.rows, a.cols, splat=splat, occlusion_tol=tol), a.reps)
                row = {'points': n, 'cams': n_cams, 'rows': a.rows, 'cols': a.cols, 'splat': splat, 'occlusion_tol': tol,
                       'render_ms': float(np.median(ms)), 'render_ms_all': ms,
                       'pairs_per_s': n * n_cams / (float(np.median(ms)) * 1e-3),
                       'covered_share': float((depth > 0).double().mean())}
                if not a.skip_host:
                    k = min(a.host_cams, n_cams)
                    t0 = time.perf_counter()
                    want = SR.scan_render(P, cams[:k], a.rows, a.cols, 0.0, splat, tol)
                    host = time.perf_counter() - t0
                    in_view = 0
                    for c in cams[:k]:
                        c2, xs, ys = SR.project(P, c, 0.0)
                        in_view += int(((c2 > 0) & (xs >= 0) & (xs < a.cols) & (ys >= 0) & (ys < a.rows)).sum())
                    same = bool(np.array_equal(depth[:k].cpu().numpy(), want))
                    row.update(numpy_s=host * n_cams / k, numpy_cams_measured=k, in_view_share=in_view / float(n * k),
                               comparator='numpy restatement (float64, np.minimum.at), one camera at a time, scaled from %d cameras' % k,
                               agrees_with_comparator=same)
                    if not same:
                        raise SystemExit('the GPU result disagrees with the restatement')
                print(json.dumps({k: v for k, v in row.items() if not k.endswith('_all')}), flush=True)
                results.append(row)
                del depth
        del dP
        torch.cuda.empty_cache()
    summary = {'parent_commit': measured_head(), 'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'results': results}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
