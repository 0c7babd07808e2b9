"""Depth-normal rates: atvs_depth_normals_f32 against its numpy restatement, and its share of SceneFusion.run.

A synthetic N-view plane scene (tools_dev/fusion_rate.py's) at each size of --sizes (views x rows x cols), every map staged with
SceneFusion.add as a network output.  Per size, after one warm-up each:

    kernel           ops.depth_normals over the staged slab, --inner launches between two device events, --reps times: the median
                     per launch (event time of back-to-back launches: the kernel plus its launch gap; --kernel-stats merges the
                     kernel's own time from a rocprofv3 --kernel-trace --stats --output-format csv run of this tool per size, kept under
                     <DIR>/<views>x<rows>x<cols>/)
    numpy            tests/depth_normals_restated.depth_normals on the host, once: the same float64 expression vectorised
    run fake/depth   SceneFusion.run() with normals='fake' and normals='depth' (host clock around work that ends in the download of
                     the points), alternating, --reps times each: medians, every sample, and the spread (inter-quartile range / median)

and the kernel's normals are compared with the restatement (largest component difference, zero patterns).  The clocks rocm-smi
shows before and after are kept as text.

--fake-only measures run fake alone and prints one JSON line; --root DIR takes the package from another checkout of the project
(a built tree of the parent commit), which need not know the normal options.  --parent-root DIR runs `--fake-only` children on
this tree and on DIR alternately, --rounds times, and records both: the one comparison with the parent.

    python tools_dev/normals_rate.py --out profiles/depth_normals.json [--parent-root DIR] [--kernel-stats DIR]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = '64x128x160,64x296x400'


def _clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=30)
        return [l for l in r.stdout.decode('utf-8', 'replace').splitlines() if 'clk' in l.lower() or 'clock' in l.lower()][:24]
    except (OSError, subprocess.SubprocessError) as e:
        return ['not available: %s' % e]


def _spread(samples):
    """The run-to-run spread of a set of samples: its inter-quartile range over its median."""
    q1, q3 = np.percentile(samples, [25, 75])
    return float(q3 - q1) / float(np.median(samples))


def _stage(DF, scene, n, rows, cols, dev, **options):
    cams, inv, prob, images = scene
    fusion = DF.SceneFusion(n, rows, cols, dev, prob_threshold=0.8, disp_threshold=0.01, num_consistent=2, inverse_depth=True, **options)
    for i in range(n):
        fusion.add(i, inv[i], prob[i], images[i], cams[i])
    return fusion


def _time_runs(torch, fusions, reps):
    """run() of each fusion in turn, reps times after one warm-up -> {name: [ms]}"""
    times = {name: [] for name in fusions}
    for name, f in fusions.items():
        f.run()
    for _ in range(reps):
        for name, f in fusions.items():
            f.result = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f.run()
            times[name].append(1e3 * (time.perf_counter() - t0))
    return times


def kernel_stats(path):
    rows = []
    for f in sorted(glob.glob(os.path.join(path, '**', '*kernel_stats.csv'), recursive=True)):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if 'depth_normals' in r['Name'] or 'fusion_' in r['Name']:
                    rows.append({'name': r['Name'], 'calls': int(r['Calls']), 'total_ms': float(r['TotalDurationNs']) / 1e6,
                                 'average_us': float(r['AverageNs']) / 1e3})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default=SIZES)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--compare-reps', type=int, default=31, help='--parent-root: runs per child process')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--fake-only', action='store_true')
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--no-numpy', action='store_true', help='skip the host restatement (profiled runs)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(HERE, 'tools_dev'))
    import torch
    import atvsnet_amd  # noqa: F401
    from atvsnet_amd import ops
    from atvsnet_amd.atvsnet import depth_fusion as DF
    from fusion_rate import plane_scene
    assert os.path.abspath(DF.__file__).startswith(root + os.sep), DF.__file__
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    sizes = [tuple(int(v) for v in s.split('x')) for s in a.sizes.split(',')]
    clocks_before = _clocks()
    results = []
    for n, rows, cols in sizes:
        scene = plane_scene(n, rows, cols)
        row = {'views': n, 'rows': rows, 'cols': cols}
        if a.fake_only:
            times = _time_runs(torch, {'fake': _stage(DF, scene, n, rows, cols, dev)}, a.reps)
            row.update(run_fake_ms=float(np.median(times['fake'])), run_fake_ms_all=times['fake'], run_fake_spread=_spread(times['fake']))
            results.append(row)
            continue
        fusions = {'fake': _stage(DF, scene, n, rows, cols, dev), 'depth': _stage(DF, scene, n, rows, cols, dev, normals='depth')}
        torch.cuda.synchronize()
        slab = fusions['depth'].nd.clone()
        cams = torch.from_numpy(np.ascontiguousarray(fusions['depth'].cams)).to(dev)
        ops.depth_normals(cams, slab)                            # warm-up
        torch.cuda.synchronize()
        per_launch = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                ops.depth_normals(cams, slab)
            e1.record()
            e1.synchronize()
            per_launch.append(1e3 * e0.elapsed_time(e1) / a.inner)
        row.update(kernel_us=float(np.median(per_launch)), kernel_us_all=per_launch, kernel_spread=_spread(per_launch),
                   pixels=n * rows * cols, pixels_per_us=n * rows * cols / float(np.median(per_launch)))
        got = slab.cpu().numpy()
        if not a.no_numpy:
            sys.path.insert(0, os.path.join(HERE, 'tests'))
            import depth_normals_restated as R
            t0 = time.perf_counter()
            want = R.depth_normals(fusions['depth'].cams, got[..., 3])
            row['numpy_ms'] = 1e3 * (time.perf_counter() - t0)
            row['numpy_over_kernel'] = row['numpy_ms'] * 1e3 / row['kernel_us']
            row['largest_component_difference'] = float(np.abs(got[..., :3].astype(np.float64) - want).max())
            row['zero_patterns_equal'] = bool(np.array_equal((got[..., :3] == 0).all(-1), (want == 0).all(-1)))
        times = _time_runs(torch, fusions, a.reps)
        for name in ('fake', 'depth'):
            row['run_%s_ms' % name] = float(np.median(times[name]))
            row['run_%s_ms_all' % name] = times[name]
            row['run_%s_spread' % name] = _spread(times[name])
            row['points_%s' % name] = int(len(fusions[name].run()[0]))
        row['kernel_share_of_run_depth'] = row['kernel_us'] / 1e3 / row['run_depth_ms']
        if a.kernel_stats:
            row['kernels'] = kernel_stats(os.path.join(a.kernel_stats, '%dx%dx%d' % (n, rows, cols)))
        results.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith('_all') and k != 'kernels'}), flush=True)
        del fusions, slab
    if a.fake_only:
        print('FAKE_ONLY ' + json.dumps(results), flush=True)
        return
    summary = {'device': torch.cuda.get_device_name(dev), 'reps': a.reps, 'inner': a.inner, 'normal_step': 1, 'normal_depth_gate': 0.02,
               'normal_threshold_deg': DF.DEPTH_NORMAL_THRESHOLD_DEG, 'disp_threshold': 0.01, 'num_consistent': 2,
               'clocks_before': clocks_before, 'results': results}
    if a.parent_root:
        # the one comparison with the parent: run fake, this tree and the parent's alternately, each in a fresh process
        compare = {'this': [], 'parent': []}
        for _ in range(a.rounds):
            for name, tree in (('this', HERE), ('parent', os.path.abspath(a.parent_root))):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--root', tree, '--fake-only', '--sizes', a.sizes,
                                    '--reps', str(a.compare_reps)], stdout=subprocess.PIPE, timeout=600, check=True)
                line = [l for l in r.stdout.decode().splitlines() if l.startswith('FAKE_ONLY ')][-1]
                compare[name].append(json.loads(line[len('FAKE_ONLY '):]))
        summary['run_fake_against_parent'] = compare
    summary['clocks_after'] = _clocks()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1)


if __name__ == '__main__':
    main()
