"""Mesh topology rates (csrc/mesh_topology.hip, atvsnet/clean_mesh.py) beside the numpy restatement and the host edge census that
mesh_fusion.mesh_report ran before the device one.

The scene is tools_dev/mesh_rate.py's: the analytic sphere in --maps (64) ring cameras of --rows x --cols (296 x 400), voxel --voxel
(0.006), meshed by ops.tsdf_integrate and ops.tsdf_mesh.  --shells (300) small closed octahedra are appended off the surface, so
that there is something to remove.

    kernels   HIP events around ops.mesh_edge_census, ops.mesh_components and ops.mesh_select (keep_largest=1's flags), each with
              its scratch allocation and its one read-back, medians of --reps after a warm-up; clean_mesh.clean_device end to end.
              On the same mesh in the same process, wall clock on one host thread: tests/mesh_topology_restated.py's edge_census,
              components and select, and mesh_fusion.host_boundary_edges (numpy.unique over all 3F edges, what mesh_report ran on
              the host for every mesh before).  The device results are compared with the host ones.
    scene     mesh_fusion.SceneMesh.run() on a depth_fusion.SceneFusion staged with the same maps: seconds['report'] (the device
              census inside mesh_report), medians of --reps after a warm-up, beside mesh_report on the same tensors moved to the
              host (the parent commit's path) timed the same way in the same run.

Each step runs as a child process under its own time limit, one after the other; the first that fails ends the run.

    python tools_dev/mesh_clean_rate.py --out profiles/mesh_clean.json
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
import mesh_topology_restated as T  # noqa: E402
import mesh_rate  # noqa: E402
from fusion_rate import measured_head  # noqa: E402
from mesh_topology_cases import OCTAHEDRON_F, OCTAHEDRON_V  # noqa: E402

STEPS = (('kernels', 400), ('scene', 300))
MEASURED = ('a-tvsnet_amd/csrc/mesh_topology.hip', 'a-tvsnet_amd/csrc/cloud_scan.h', 'a-tvsnet_amd/ops/mesh_topology.py',
            'a-tvsnet_amd/atvsnet/clean_mesh.py', 'a-tvsnet_amd/atvsnet/mesh_fusion.py')


def sources_sha1():
    import hashlib
    h = hashlib.sha1()
    for p in MEASURED:
        with open(os.path.join(ROOT, p), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def _wall(fn, reps):
    out, times = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times)), times


def step_kernels(a):
    import torch
    from atvsnet_amd import ops
    from atvsnet_amd.atvsnet import clean_mesh, mesh_fusion
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = mesh_rate.scene(a)
    d, c, im = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams, images))
    volume = ops.tsdf_integrate(d, c, a.voxel, trunc, origin, dims, images=im, max_blocks=a.max_blocks)
    vertices, colors, faces = (t.cpu().numpy() for t in ops.tsdf_mesh(volume, a.min_weight))
    sphere_faces = len(faces)
    rng = np.random.RandomState(11)
    vs, cs, fs = [vertices], [colors], [faces]
    for k in range(a.shells):                            # closed shells of 8 faces between 1.15 and 1.4 radii from the centre
        direction = rng.standard_normal(3)
        centre = direction / np.linalg.norm(direction) * mesh_rate.RADIUS * rng.uniform(1.15, 1.4)
        fs.append((OCTAHEDRON_F + sum(len(v) for v in vs)).astype(np.int32))
        vs.append((centre + 2.0 * a.voxel * OCTAHEDRON_V).astype(np.float32))
        cs.append(np.full((6, 3), 200, np.uint8))
    vertices, colors, faces = np.concatenate(vs), np.concatenate(cs), np.concatenate(fs)
    nv, nf = len(vertices), len(faces)
    dv, dc, df = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (vertices, colors, faces))
    ms, ms_all, host_s, host_all = {}, {}, {}, {}

    def timed(name, fn):
        out, ms[name], ms_all[name] = mesh_rate._median_ms(fn, a.reps)
        return out

    def hosted(name, fn, reps):
        out, host_s[name], host_all[name] = _wall(fn, reps)
        return out

    census = timed('mesh_edge_census', lambda: ops.mesh_edge_census(df, nv))
    comps = timed('mesh_components', lambda: ops.mesh_components(df, nv))
    keep = clean_mesh.keep_components(comps[2].cpu().numpy(), keep_largest=1)
    flags = torch.from_numpy(keep.astype(np.uint8)).to(dev)[comps[1].long()].contiguous()
    selected = timed('mesh_select', lambda: ops.mesh_select(dv, dc, df, flags))
    cleaned = timed('clean_device', lambda: clean_mesh.clean_device(dv, dc, df, keep_largest=1))
    # the host forms, on the same mesh
    f64 = faces.astype(np.int64)
    old_boundary = hosted('mesh_report_host_census', lambda: mesh_fusion.host_boundary_edges(f64, nv), a.reps)
    want_census = hosted('restated_edge_census', lambda: T.edge_census(faces, nv), a.reps)
    want_comps = hosted('restated_components', lambda: T.components(faces, nv), 1)
    want_select = hosted('restated_select', lambda: T.select(vertices, colors, faces, flags.cpu().numpy()), a.reps)
    assert census == want_census and census['boundary'] == old_boundary, (census, want_census, old_boundary)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(comps, want_comps))
    assert all(np.array_equal(g.cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8)) for g, w in zip(selected, want_select))
    largest = int(want_comps[2].max())                  # the meshed sphere may itself carry fragments: they go too
    assert cleaned[3]['components_removed'] == len(want_comps[2]) - 1 >= a.shells and cleaned[3]['faces_out'] == largest <= sphere_faces
    return {'device': torch.cuda.get_device_name(dev), 'vertices': nv, 'faces': nf, 'sphere_faces': sphere_faces, 'shells': a.shells,
            'components': int(len(want_comps[2])), 'census': census, 'ms': ms, 'ms_all': ms_all, 'host_s': host_s, 'host_s_all': host_all,
            'clean_report': cleaned[3],
            'census_faces_per_s': nf / (ms['mesh_edge_census'] * 1e-3), 'components_faces_per_s': nf / (ms['mesh_components'] * 1e-3),
            'census_speedup_over_host': host_s['mesh_report_host_census'] / (ms['mesh_edge_census'] * 1e-3)}


def step_scene(a):
    import torch
    from atvsnet_amd.atvsnet import depth_fusion as DF, mesh_fusion
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = mesh_rate.scene(a)
    n, rows, cols = depths.shape
    cam44 = np.zeros((n, 2, 4, 4))
    for k, c in enumerate(cams):
        cam44[k, 0] = np.eye(4)
        cam44[k, 0, :3, :3], cam44[k, 0, :3, 3] = c[:9].reshape(3, 3), c[9:12]
        cam44[k, 1, :3, :3] = [[c[12], 0, c[14]], [0, c[13], c[15]], [0, 0, 1]]
        cam44[k, 1, 3] = (1.0, 0.02, 128, 3.6)
    fusion = DF.SceneFusion(n, rows, cols, dev, prob_threshold=0.5, disp_threshold=0.25, num_consistent=2, inverse_depth=False)
    for k in range(n):
        fusion.add(k, np.ascontiguousarray(depths[k]), np.ones((rows, cols), np.float32), np.clip(images[k], 0, 255).astype(np.uint8), cam44[k])
    fusion.run()
    device_s, host_s, run_s = [], [], []
    for _ in range(a.reps + 1):                          # the first is the warm-up
        scene_mesh = mesh_fusion.SceneMesh(fusion, cam44, a.voxel, 4.0, a.min_weight, a.max_blocks)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scene_mesh.run()
        run_s.append(time.perf_counter() - t0)
        report = scene_mesh.report()
        device_s.append(report['seconds']['report'])
        on_host = tuple(None if t is None else t.cpu() for t in scene_mesh._device_mesh)
        t0 = time.time()                                 # as SceneMesh.run() times it
        host_report = mesh_fusion.mesh_report(scene_mesh.volume, on_host, a.min_weight, {})
        host_s.append(time.time() - t0)
        assert {k: v for k, v in host_report.items() if k != 'seconds'} == {k: v for k, v in report.items() if k != 'seconds'}
    return {'faces': report['faces'], 'vertices': report['vertices'], 'boundary_edges': report['boundary_edges'],
            'report_s_device_census': float(np.median(device_s[1:])), 'report_s_device_census_all': device_s[1:],
            'report_s_host_census': float(np.median(host_s[1:])), 'report_s_host_census_all': host_s[1:],
            'scene_mesh_run_s': float(np.median(run_s[1:])), 'scene_mesh_run_s_all': run_s[1:], 'seconds': report['seconds']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--rows', type=int, default=296)
    ap.add_argument('--cols', type=int, default=400)
    ap.add_argument('--voxel', type=float, default=0.006)
    ap.add_argument('--min_weight', type=float, default=2.0)
    ap.add_argument('--max_blocks', type=int, default=131072)
    ap.add_argument('--shells', type=int, default=300)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--step', default=None, choices=[s for s, _ in STEPS], help='run one step in this process and write its result to --out')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.step is not None:
        result = {'kernels': step_kernels, 'scene': step_scene}[a.step](a)
        print(json.dumps({k: v for k, v in result.items() if not k.endswith('_all')}), flush=True)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(result, f)
        return 0
    summary = {'parent_commit': measured_head(), 'sources_sha1': sources_sha1(),
               'scene': {'maps': a.maps, 'rows': a.rows, 'cols': a.cols, 'voxel': a.voxel, 'trunc_voxels': 4.0, 'min_weight': a.min_weight,
                         'sphere_radius': mesh_rate.RADIUS, 'shells': a.shells, 'cameras': 'tests/scan_render_restated.ring_cameras'},
               'reps': a.reps}
    common = [x for k in ('maps', 'rows', 'cols', 'voxel', 'min_weight', 'max_blocks', 'shells', 'reps') for x in ('--' + k, str(getattr(a, k)))]
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:                        # one after the other: a step that fails or runs out of time ends the run
            part = os.path.join(tmp, step + '.json')
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--out', part] + common, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print('mesh_clean_rate: step %s ended with %d: nothing further is run' % (step, rc), file=sys.stderr)
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
