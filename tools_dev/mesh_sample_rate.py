"""Surface sampling rates (csrc/mesh_sample.hip, ops/mesh_sample.py) beside the numpy restatement.

The mesh is tools_dev/mesh_rate.py's: the analytic sphere in --maps (64) ring cameras of --rows x --cols (296 x 400), voxel --voxel
(0.006), meshed by ops.tsdf_integrate and ops.tsdf_mesh: about 2.3 M faces.  Its surface is sampled at a spacing of
--spacing_voxels (0.5) voxels: about half a sample per face, the case stochastic rounding exists for.

    kernels   HIP events around atvs_mesh_sample_counts, atvs_mesh_sample_offsets (the scan) and atvs_mesh_sample_place, each on
              buffers made beforehand (--inner (20) back-to-back calls between one pair of events, per call: one call is tens of
              microseconds), and around ops.mesh_sample end to end (its allocations and its two read-backs included) with
              colours and normals; medians of --reps after a warm-up, every run kept.  On the same mesh in the same process, wall clock
              on one host thread, once: counts, offsets and place of tests/mesh_sample_restated.py.  The device's counts are compared
              with the host's on the faces whose rounding is sure, and the samples bit for bit where all are.

The step runs as a child process under its own time limit; a step that fails ends the run.

    python tools_dev/mesh_sample_rate.py --out profiles/mesh_sample.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import atvsnet_amd  # noqa: E402,F401
import mesh_sample_restated as R  # noqa: E402
import mesh_rate  # noqa: E402
from fusion_rate import measured_head  # noqa: E402

STEPS = (('kernels', 500),)
MEASURED = ('a-tvsnet_amd/csrc/mesh_sample.hip', 'a-tvsnet_amd/csrc/cloud_scan.h', 'a-tvsnet_amd/ops/mesh_sample.py')


def sources_sha1():
    import hashlib
    h = hashlib.sha1()
    for p in MEASURED:
        with open(os.path.join(ROOT, p), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def _once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def step_kernels(a):
    import torch
    from atvsnet_amd import ops
    from atvsnet_amd.ops.base import _call, _p, _size, _stream
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = mesh_rate.scene(a)
    d, c, im = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams, images))
    volume = ops.tsdf_integrate(d, c, a.voxel, trunc, origin, dims, images=im, max_blocks=a.max_blocks)
    dv, dc, df = (t.contiguous() for t in ops.tsdf_mesh(volume, a.min_weight))
    vertices, colors, faces = (t.cpu().numpy() for t in (dv, dc, df))
    nv, nf = len(vertices), len(faces)
    spacing = a.spacing_voxels * a.voxel
    density = 1.0 / (spacing * spacing)
    ms, ms_all, host_s, spread = {}, {}, {}, {}

    def timed(name, fn, inner=1):
        """The median of --reps timings of `inner` back-to-back calls between one pair of events, per call; every run is kept."""
        def many():
            for _ in range(inner - 1):
                fn()
            return fn()
        out, _, times = mesh_rate._median_ms(many, a.reps)
        ms_all[name] = [t / inner for t in times]
        ms[name] = float(np.median(ms_all[name]))
        spread[name] = [float(min(ms_all[name])), float(max(ms_all[name]))]
        return out

    def hosted(name, fn):
        out, host_s[name] = _once(fn)
        return out

    counts = torch.empty(nf, dtype=torch.int32, device=dev)
    areas = torch.empty(nf, dtype=torch.float64, device=dev)
    words = torch.empty(4, dtype=torch.int64, device=dev)
    timed('counts', lambda: _call('atvs_mesh_sample_counts', _p(dv), nv, _p(df), nf, density, a.seed, _p(counts), _p(areas), _p(words), _stream()), a.inner)
    total = int(words[0].item())
    scratch = torch.empty(_size('atvs_mesh_sample_scratch_size', nf), dtype=torch.uint8, device=dev)
    offsets = torch.empty(nf + 1, dtype=torch.int32, device=dev)
    timed('scan', lambda: _call('atvs_mesh_sample_offsets', _p(counts), nf, _p(scratch), scratch.numel(), _p(offsets), _stream()), a.inner)
    points = torch.empty((total, 3), dtype=torch.float32, device=dev)
    face = torch.empty(total, dtype=torch.int32, device=dev)
    out_c = torch.empty((total, 3), dtype=torch.uint8, device=dev)
    normals = torch.empty((total, 3), dtype=torch.float32, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    timed('place', lambda: _call('atvs_mesh_sample_place', _p(dv), _p(dc), nv, _p(df), nf, _p(offsets), total, a.seed, _p(points), _p(face),
                                 _p(out_c), _p(normals), _p(info), _stream()), a.inner)
    timed('place_points_only', lambda: _call('atvs_mesh_sample_place', _p(dv), None, nv, _p(df), nf, _p(offsets), total, a.seed, _p(points),
                                             _p(face), None, None, _p(info), _stream()), a.inner)
    assert info.cpu().tolist() == [0, 0]
    whole = timed('mesh_sample', lambda: ops.mesh_sample(dv, dc, df, density, a.seed, normals=True))
    ops.mesh_sample(dv, dc, df, density, a.seed, normals=True)
    runs = [_once(lambda: (ops.mesh_sample(dv, dc, df, density, a.seed, normals=True), torch.cuda.synchronize())[0]) for _ in range(a.reps)]
    wall = [s for _, s in runs]
    # the restatement, on the same mesh
    want_c = hosted('counts', lambda: R.counts(vertices, faces, density, a.seed))
    hosted('scan', lambda: R.offsets(want_c['counts']))
    sure = want_c['margin'] >= R.SURE
    got_counts = counts.cpu().numpy()
    assert np.array_equal(got_counts[sure], want_c['counts'][sure])
    want_p = hosted('place', lambda: R.place(vertices, colors, faces, got_counts, a.seed))
    host_s['whole'] = host_s['counts'] + host_s['scan'] + host_s['place']
    same = lambda g, w: np.array_equal(g.cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8))          # noqa: E731
    assert same(whole[0].points, want_p['points']) and same(whole[0].face, want_p['face']) and same(whole[0].colors, want_p['colors'])
    normal_error = float(np.abs(whole[0].normals.cpu().numpy().astype(np.float64) - want_p['normals'].astype(np.float64)).max())
    radius = np.linalg.norm(want_p['points'].astype(np.float64), axis=1)
    stages = ms['counts'] + ms['scan'] + ms['place']
    out_bytes = total * (12 + 4 + 3 + 12)
    return {'device': torch.cuda.get_device_name(dev), 'vertices': nv, 'faces': nf, 'spacing': spacing, 'spacing_voxels': a.spacing_voxels,
            'density': density, 'seed': a.seed, 'samples': total, 'expected_samples': float(want_c['x'].sum()), 'info': whole[1],
            'unsure_faces': int((~sure).sum()), 'smallest_margin': float(want_c['margin'].min()), 'ms': ms, 'ms_min_max': spread, 'inner': a.inner, 'ms_all': ms_all, 'host_s': host_s,
            'mesh_sample_wall_s': float(np.median(wall)), 'mesh_sample_wall_s_all': wall, 'stages_ms': stages,
            'faces_per_s_counts': nf / (ms['counts'] * 1e-3), 'faces_per_s_scan': nf / (ms['scan'] * 1e-3),
            'samples_per_s_place': total / (ms['place'] * 1e-3), 'samples_per_s_mesh_sample': total / (ms['mesh_sample'] * 1e-3),
            'place_output_gb_per_s': out_bytes / (ms['place'] * 1e-3) / 1e9, 'speedup_over_restatement': host_s['whole'] / (stages * 1e-3),
            'largest_normal_difference': normal_error,
            'sphere': {'mean_radius_error': float(radius.mean() - mesh_rate.RADIUS), 'max_radius_error': float(np.abs(radius - mesh_rate.RADIUS).max())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--rows', type=int, default=296)
    ap.add_argument('--cols', type=int, default=400)
    ap.add_argument('--voxel', type=float, default=0.006)
    ap.add_argument('--min_weight', type=float, default=2.0)
    ap.add_argument('--max_blocks', type=int, default=131072)
    ap.add_argument('--spacing_voxels', type=float, default=0.5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20, help='back-to-back calls of an entry point between one pair of events')
    ap.add_argument('--step', default=None, choices=[s for s, _ in STEPS], help='run one step in this process and write its result to --out')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.step is not None:
        result = {'kernels': step_kernels}[a.step](a)
        print(json.dumps({k: v for k, v in result.items() if not k.endswith('_all')}), flush=True)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(result, f)
        return 0
    summary = {'parent_commit': measured_head(), 'sources_sha1': sources_sha1(),
               'scene': {'maps': a.maps, 'rows': a.rows, 'cols': a.cols, 'voxel': a.voxel, 'trunc_voxels': 4.0, 'min_weight': a.min_weight,
                         'sphere_radius': mesh_rate.RADIUS, 'spacing_voxels': a.spacing_voxels, 'cameras': 'tests/scan_render_restated.ring_cameras'},
               'reps': a.reps, 'inner': a.inner}
    common = [x for k in ('maps', 'rows', 'cols', 'voxel', 'min_weight', 'max_blocks', 'spacing_voxels', 'seed', 'reps', 'inner')
              for x in ('--' + k, str(getattr(a, k)))]
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:                        # a step that fails or runs out of time ends the run
            part = os.path.join(tmp, step + '.json')
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--out', part] + common, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print('mesh_sample_rate: step %s ended with %d: nothing further is run' % (step, rc), file=sys.stderr)
                return rc
            with open(part) as f:
                summary[step] = json.load(f)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(summary, f, indent=1, sort_keys=True)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
