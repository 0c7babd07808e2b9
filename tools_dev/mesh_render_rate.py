"""Mesh rendering rates (csrc/mesh_render.hip) in its two regimes, beside the scan renderer and the numpy restatement.

    subpixel     the TSDF sphere mesh of tools_dev/mesh_rate.py (radius 0.9, voxel 0.006: about 2.3 M faces, each under a pixel)
                 rendered into its --maps (64) ring cameras of --rows x --cols (296 x 400): the small path, one lane per face.
                 Beside it ops.scan_render of the same mesh's vertices at splat 0 into the same cameras: the project's existing
                 renderer on the same scene.
    large        --large (300) triangles of about an image's size around the same ring, a part of them crossing camera planes:
                 the large path, a workgroup per (face, camera, 64 x 64 tile).
    restatement  tests/mesh_render_restated.py (numpy, dense, one thread per camera) on a sub-problem: --host_faces faces of the
                 sphere mesh's own kind into --host_maps cameras of a quarter of the size, as face-pixel tests per second.

atvs_mesh_render and atvs_scan_render are timed with HIP events around the entry point alone (buffers allocated before), medians of
--reps after a warm-up.  Each step runs as a child process under its own time limit, one after the other; the first that fails ends
the run.  No counter run is made here.

    python tools_dev/mesh_render_rate.py --out profiles/mesh_render.json
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
import mesh_render_restated as MR  # noqa: E402
from fusion_rate import measured_head  # noqa: E402
import mesh_rate  # noqa: E402

STEPS = (('subpixel', 400), ('large', 200), ('restatement', 200))
MEASURED = ('a-tvsnet_amd/csrc/mesh_render.hip', 'a-tvsnet_amd/csrc/scan_project.h', 'a-tvsnet_amd/csrc/cloud_scan.h',
            'a-tvsnet_amd/ops/mesh.py')


def sources_sha1():
    import hashlib
    h = hashlib.sha1()
    for p in MEASURED:
        with open(os.path.join(ROOT, p), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def _render_ms(v, f, c, rows, cols, reps):
    """atvs_mesh_render alone -> (depth, face, median ms, all ms)."""
    import torch
    from atvsnet_amd.ops.base import _call, _p, _size, _stream
    n = int(c.shape[0])
    depth = torch.empty((n, rows, cols), dtype=torch.float32, device=v.device)
    face = torch.empty((n, rows, cols), dtype=torch.int32, device=v.device)
    scratch = torch.empty(_size('atvs_mesh_render_scratch_size', n, rows, cols, int(f.shape[0])), dtype=torch.uint8, device=v.device)
    err = torch.empty(1, dtype=torch.int32, device=v.device)
    _, ms, every = mesh_rate._median_ms(lambda: _call('atvs_mesh_render', _p(v), int(v.shape[0]), _p(f), int(f.shape[0]), _p(c), n, rows,
                                                      cols, 0.0, _p(scratch), scratch.numel(), _p(depth), _p(face), _p(err), _stream()), reps)
    assert int(err.item()) == 0
    return depth, face, ms, every, scratch.numel()


def step_subpixel(a):
    import torch
    from atvsnet_amd import ops
    from atvsnet_amd.ops.base import _call, _p, _size, _stream
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = mesh_rate.scene(a)
    d, c = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams))
    volume = ops.tsdf_integrate(d, c, a.voxel, trunc, origin, dims, max_blocks=a.max_blocks)
    v, _, f = ops.tsdf_mesh(volume, a.min_weight)
    n, rows, cols = depths.shape
    depth, face, ms, every, scratch = _render_ms(v, f, c, rows, cols, a.reps)
    again = ops.mesh_render(v, f, c, rows, cols)
    assert torch.equal(again[0], depth) and torch.equal(again[1], face)
    splat = torch.empty((n, rows, cols), dtype=torch.float32, device=dev)
    s2 = torch.empty(_size('atvs_scan_render_scratch_size', n, rows, cols), dtype=torch.uint8, device=dev)
    _, scan_ms, scan_every = mesh_rate._median_ms(lambda: _call('atvs_scan_render', _p(v), int(v.shape[0]), _p(c), n, rows, cols, 0.0, 0, 0.0,
                                                                _p(s2), s2.numel(), _p(splat), _stream()), a.reps)
    hit = torch.from_numpy(depths > 0).to(dev)
    pairs = int(f.shape[0]) * n
    return {'device': torch.cuda.get_device_name(dev), 'vertices': int(v.shape[0]), 'faces': int(f.shape[0]), 'maps': n, 'rows': rows,
            'cols': cols, 'scratch_bytes': int(scratch), 'mesh_render_ms': ms, 'mesh_render_ms_all': every,
            'face_camera_pairs_per_s': pairs / (ms * 1e-3), 'covered_fraction': float((depth > 0).float().mean().item()),
            'covered_of_analytic_sphere': float(((depth > 0) & hit).sum().item()) / float(hit.sum().item()),
            'scan_render_vertices_splat0_ms': scan_ms, 'scan_render_vertices_splat0_ms_all': scan_every,
            'scan_render_point_camera_pairs_per_s': int(v.shape[0]) * n / (scan_ms * 1e-3),
            'scan_render_covered_fraction': float((splat > 0).float().mean().item())}


def large_triangles(a):
    rng = np.random.default_rng(7)
    cams = MR.ring_cameras(a.maps, a.rows, a.cols)
    size = 3.0 * a.cols / cams[0, 12]                                    # an image's width at the ring's centre
    centre = rng.uniform(-3.5, 3.5, (a.large, 3))                        # a box that holds the ring of radius 3
    tri = centre[:, None, :] + rng.normal(size=(a.large, 3, 3)) * (0.5 * size * rng.uniform(0.5, 2.0, (a.large, 1, 1)))
    return cams, tri.reshape(-1, 3).astype(np.float32), np.arange(3 * a.large, dtype=np.int32).reshape(-1, 3)


def step_large(a):
    import torch
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, v, f = large_triangles(a)
    z = np.stack([MR.camera_space(v, c)[:, 2] for c in cams])[:, f.reshape(-1)].reshape(len(cams), -1, 3)
    crossing = int(((z > 0).any(2) & (z <= 0).any(2)).sum())
    vd, fd, cd = (torch.from_numpy(x).to(dev) for x in (v, f, cams))
    depth, face, ms, every, scratch = _render_ms(vd, fd, cd, a.rows, a.cols, a.reps)
    pixels = len(cams) * a.rows * a.cols
    return {'faces': int(len(f)), 'maps': len(cams), 'rows': a.rows, 'cols': a.cols, 'pairs_crossing_a_camera_plane': crossing,
            'scratch_bytes': int(scratch), 'mesh_render_ms': ms, 'mesh_render_ms_all': every,
            'covered_fraction': float((depth > 0).float().mean().item()), 'faces_shown': int(torch.unique(face).numel()) - 1,
            'face_pixel_tests_upper_bound_per_s': len(f) * pixels / (ms * 1e-3)}


def step_restatement(a):
    rows, cols = a.rows // 4, a.cols // 4
    cams = MR.ring_cameras(a.host_maps, rows, cols)
    v, f = MR.octahedron_sphere(6, 0.9)                                  # 32768 faces of about a pixel
    f = f[:a.host_faces]
    t0 = time.perf_counter()
    depth, _ = MR.mesh_render(v, f, cams, rows, cols, 0.0)
    s = time.perf_counter() - t0
    tests = len(f) * len(cams) * rows * cols
    return {'what': 'tests/mesh_render_restated.py (numpy, dense, a thread per camera)', 'faces': int(len(f)), 'maps': len(cams), 'rows': rows,
            'cols': cols, 'seconds': s, 'face_pixel_tests': tests, 'face_pixel_tests_per_s': tests / s,
            'face_camera_pairs_per_s': len(f) * len(cams) / s, 'covered_fraction': float((depth > 0).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--rows', type=int, default=296)
    ap.add_argument('--cols', type=int, default=400)
    ap.add_argument('--voxel', type=float, default=0.006)
    ap.add_argument('--min_weight', type=float, default=2.0)
    ap.add_argument('--max_blocks', type=int, default=131072)
    ap.add_argument('--large', type=int, default=300)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host_faces', type=int, default=8192)
    ap.add_argument('--host_maps', type=int, default=4)
    ap.add_argument('--step', default=None, choices=[s for s, _ in STEPS], help='run one step in this process and write its result to --out')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.step is not None:
        result = {'subpixel': step_subpixel, 'large': step_large, 'restatement': step_restatement}[a.step](a)
        print(json.dumps({k: v for k, v in result.items() if not k.endswith('_all')}), flush=True)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(result, f)
        return 0
    summary = {'parent_commit': measured_head(), 'sources_sha1': sources_sha1(), 'reps': a.reps, 'counter_run': False,
               'scene': {'maps': a.maps, 'rows': a.rows, 'cols': a.cols, 'voxel': a.voxel, 'sphere_radius': mesh_rate.RADIUS,
                         'cameras': 'tests/scan_render_restated.ring_cameras', 'large_triangles': a.large}}
    passed = ['maps', 'rows', 'cols', 'voxel', 'min_weight', 'max_blocks', 'large', 'reps', 'host_faces', 'host_maps']
    common = [x for k in passed for x in ('--' + k, str(getattr(a, k)))]
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:                        # one after the other: a step that fails or runs out of time ends the run
            part = os.path.join(tmp, step + '.json')
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--out', part] + common, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print('mesh_render_rate: step %s ended with %d: nothing further is run' % (step, rc), file=sys.stderr)
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
