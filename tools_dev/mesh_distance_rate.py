"""Point-to-triangle distance rates (csrc/mesh_distance.hip, ops/mesh_distance.py) beside the numpy restatement and beside the
sample-based route they replace.

The mesh is tools_dev/mesh_rate.py's: the analytic sphere in --maps (64) ring cameras of --rows x --cols (296 x 400), voxel --voxel
(0.006), meshed by ops.tsdf_integrate and ops.tsdf_mesh: about 2.3 M faces.  The queries are samples of its surface at a spacing of
--spacing_voxels (0.5) voxels, about 1 M, each moved by a seeded uniform offset of up to the radius per axis; the radius is
--radius_voxels (2) voxels.

    kernels   HIP events around atvs_mesh_grid_build and atvs_mesh_nearest, each on buffers made beforehand, and around ops.mesh_grid
              and ops.mesh_nearest end to end (allocations and the grid's read-back included); medians of --reps after a warm-up,
              every run kept.  ops.cloud_grid and ops.cloud_nearest of the same queries against samples of the mesh at a spacing of half
              the radius: the sample-based route.  On --host_queries (16) of the queries, wall clock on one host thread, once: the
              brute force of tests/mesh_distance_restated.py over all faces, compared with the device bit for bit.

The step runs as a child process under its own time limit; a step that fails ends the run.

    python tools_dev/mesh_distance_rate.py --out profiles/mesh_distance.json
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
import mesh_distance_restated as R  # noqa: E402
import mesh_rate  # noqa: E402
from fusion_rate import measured_head  # noqa: E402

STEPS = (('kernels', 500),)
MEASURED = ('a-tvsnet_amd/csrc/mesh_distance.hip', 'a-tvsnet_amd/csrc/cloud_grid.h', 'a-tvsnet_amd/csrc/cloud_scan.h',
            'a-tvsnet_amd/ops/mesh_distance.py')


def sources_sha1():
    import hashlib
    h = hashlib.sha1()
    for p in MEASURED:
        with open(os.path.join(ROOT, p), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def step_kernels(a):
    import torch
    from atvsnet_amd import ops
    from atvsnet_amd.ops.base import _call, _p, _size, _stream
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = mesh_rate.scene(a)
    d, c, im = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams, images))
    volume = ops.tsdf_integrate(d, c, a.voxel, trunc, origin, dims, images=im, max_blocks=a.max_blocks)
    dv, _, df = (t.contiguous() for t in ops.tsdf_mesh(volume, a.min_weight))
    nv, nf = int(dv.shape[0]), int(df.shape[0])
    radius = float(np.float32(a.radius_voxels * a.voxel))
    spacing = a.spacing_voxels * a.voxel
    on_surface = ops.mesh_sample(dv, None, df, 1.0 / (spacing * spacing), a.seed)[0].points
    m = int(on_surface.shape[0])
    offsets = np.random.RandomState(a.seed).uniform(-radius, radius, (m, 3)).astype(np.float32)
    queries = (on_surface + torch.from_numpy(offsets).to(dev)).contiguous()
    ms, ms_all, spread = {}, {}, {}

    def timed(name, fn):
        out, _, times = mesh_rate._median_ms(fn, a.reps)
        ms_all[name], ms[name], spread[name] = times, float(np.median(times)), [float(min(times)), float(max(times))]
        return out

    grid = timed('mesh_grid', lambda: ops.mesh_grid(dv, df, radius))
    info = torch.empty(4, dtype=torch.int64, device=dev)
    buf = torch.empty(_size('atvs_mesh_grid_scratch_size', nf, grid.max_refs), dtype=torch.uint8, device=dev)
    timed('grid_build', lambda: _call('atvs_mesh_grid_build', _p(dv), nv, _p(df), nf, radius, 0.0, grid.max_refs, _p(buf), buf.numel(),
                                      _p(info), _stream()))
    d2 = torch.empty(m, dtype=torch.float32, device=dev)
    face = torch.empty(m, dtype=torch.int32, device=dev)
    closest = torch.empty((m, 3), dtype=torch.float32, device=dev)
    scratch = torch.empty(_size('atvs_mesh_nearest_scratch_size', nf, m), dtype=torch.uint8, device=dev)
    timed('nearest', lambda: _call('atvs_mesh_nearest', _p(buf), buf.numel(), nf, grid.max_refs, _p(queries), m, _p(scratch),
                                   scratch.numel(), _p(d2), _p(face), None, _stream()))
    timed('nearest_with_closest', lambda: _call('atvs_mesh_nearest', _p(buf), buf.numel(), nf, grid.max_refs, _p(queries), m, _p(scratch),
                                                scratch.numel(), _p(d2), _p(face), _p(closest), _stream()))
    got = timed('mesh_nearest', lambda: ops.mesh_nearest(grid, queries))
    assert torch.equal(got[0], d2) and torch.equal(got[1], face)
    # the sample-based route: the same queries against samples of the mesh at half the radius
    half = 0.5 * radius
    samples = timed('mesh_sample_half_radius', lambda: ops.mesh_sample(dv, None, df, 1.0 / (half * half), a.seed)[0].points)
    cgrid = timed('cloud_grid', lambda: ops.cloud_grid(samples, radius))
    s2, _ = timed('cloud_nearest', lambda: ops.cloud_nearest(cgrid, queries))
    e, s = np.sqrt(d2.cpu().numpy().astype(np.float64)), np.sqrt(s2.cpu().numpy().astype(np.float64))
    both = np.isfinite(e) & np.isfinite(s)
    # the restatement on a few queries, by brute force over all faces
    rows = np.random.RandomState(a.seed + 1).choice(m, a.host_queries, replace=False)
    vertices, faces, q = dv.cpu().numpy(), df.cpu().numpy(), queries.cpu().numpy()
    t0 = time.perf_counter()
    want = R.nearest(vertices, faces, q[rows], radius)
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(want[0].view(np.uint32), d2.cpu().numpy()[rows].view(np.uint32)) and
                np.array_equal(want[1], face.cpu().numpy()[rows]))
    assert same, 'the device and the restatement differ on the %d host queries' % a.host_queries
    return {'device': torch.cuda.get_device_name(dev), 'vertices': nv, 'faces': nf, 'usable_faces': grid.usable_faces, 'queries': m,
            'radius': radius, 'radius_voxels': a.radius_voxels, 'query_spacing': spacing, 'cell': grid.cell, 'references': grid.refs,
            'references_per_face': grid.refs / float(max(nf, 1)), 'max_refs': grid.max_refs, 'builds': grid.rounds,
            'grid_bytes': int(buf.numel()), 'found': int(np.isfinite(e).sum()), 'ms': ms, 'ms_min_max': spread, 'ms_all': ms_all,
            'queries_per_s_nearest': m / (ms['nearest'] * 1e-3), 'faces_per_s_grid_build': nf / (ms['grid_build'] * 1e-3),
            'host_queries': a.host_queries, 'host_s': host_s, 'host_s_per_query': host_s / a.host_queries, 'host_matches_device_bits': same,
            'speedup_over_restatement_per_query': (host_s / a.host_queries) / (ms['nearest'] * 1e-3 / m),
            'samples_route': {'spacing': half, 'samples': int(samples.shape[0]), 'found': int(np.isfinite(s).sum()),
                              'ms_total': ms['mesh_sample_half_radius'] + ms['cloud_grid'] + ms['cloud_nearest'],
                              'mean_excess_of_sample_distance': float((s[both] - e[both]).mean()),
                              'max_excess_of_sample_distance': float((s[both] - e[both]).max()),
                              'min_excess_of_sample_distance': float((s[both] - e[both]).min())},
            'exact_route_ms_total': ms['mesh_grid'] + ms['mesh_nearest']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--rows', type=int, default=296)
    ap.add_argument('--cols', type=int, default=400)
    ap.add_argument('--voxel', type=float, default=0.006)
    ap.add_argument('--min_weight', type=float, default=2.0)
    ap.add_argument('--max_blocks', type=int, default=131072)
    ap.add_argument('--spacing_voxels', type=float, default=0.5)
    ap.add_argument('--radius_voxels', type=float, default=2.0)
    ap.add_argument('--host_queries', type=int, default=16)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--reps', type=int, default=9)
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
                         'sphere_radius': mesh_rate.RADIUS, 'spacing_voxels': a.spacing_voxels, 'radius_voxels': a.radius_voxels,
                         'cameras': 'tests/scan_render_restated.ring_cameras'},
               'reps': a.reps}
    common = [x for k in ('maps', 'rows', 'cols', 'voxel', 'min_weight', 'max_blocks', 'spacing_voxels', 'radius_voxels', 'host_queries',
                          'seed', 'reps') for x in ('--' + k, str(getattr(a, k)))]
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:                        # a step that fails or runs out of time ends the run
            part = os.path.join(tmp, step + '.json')
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--out', part] + common, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print('mesh_distance_rate: step %s ended with %d: nothing further is run' % (step, rc), file=sys.stderr)
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
