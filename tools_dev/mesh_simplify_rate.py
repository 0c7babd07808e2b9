"""Mesh simplification rates (csrc/mesh_simplify.hip, atvsnet/simplify_mesh.py) beside the numpy restatement.

The mesh is tools_dev/mesh_rate.py's: the analytic sphere in --maps (64) ring cameras of --rows x --cols (296 x 400), voxel --voxel
(0.006), meshed by ops.tsdf_integrate and ops.tsdf_mesh: about 2.3 M faces.  It is simplified on cells of --cell_voxels (4) voxels
whose origin is the volume's, as SceneMesh(simplify=) does.

    kernels   HIP events around each stage as simplify_device calls it -- ops.mesh_cluster, ops.mesh_cluster_quadrics,
              ops.mesh_cluster_place, ops.mesh_cluster_max_move, ops.mesh_cluster_faces, ops.mesh_select -- each with its scratch
              allocation and its read-back, medians of --reps after a warm-up; simplify_mesh.simplify_device end to end for both
              placements (with its two edge censuses), wall clock.  On the same mesh in the same process, wall clock on one host
              thread, once: the stages of tests/mesh_simplify_restated.py.  The device results are compared with the host ones.

The step runs as a child process under its own time limit; a step that fails ends the run.

    python tools_dev/mesh_simplify_rate.py --out profiles/mesh_simplify.json
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
import mesh_simplify_restated as S  # noqa: E402
import mesh_topology_restated as T  # noqa: E402
import mesh_rate  # noqa: E402
from fusion_rate import measured_head  # noqa: E402

STEPS = (('kernels', 500),)
MEASURED = ('a-tvsnet_amd/csrc/mesh_simplify.hip', 'a-tvsnet_amd/csrc/jacobi3.h', 'a-tvsnet_amd/csrc/cloud_voxel.h',
            'a-tvsnet_amd/csrc/cloud_scan.h', 'a-tvsnet_amd/csrc/mesh_topology.hip', 'a-tvsnet_amd/ops/mesh_simplify.py',
            'a-tvsnet_amd/atvsnet/simplify_mesh.py')


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
    from atvsnet_amd.atvsnet import simplify_mesh
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = mesh_rate.scene(a)
    d, c, im = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams, images))
    volume = ops.tsdf_integrate(d, c, a.voxel, trunc, origin, dims, images=im, max_blocks=a.max_blocks)
    dv, dc, df = ops.tsdf_mesh(volume, a.min_weight)
    vertices, colors, faces = (t.cpu().numpy() for t in (dv, dc, df))
    nv, nf = len(vertices), len(faces)
    cell, org = a.cell_voxels * a.voxel, tuple(float(o) for o in volume.origin)
    ms, ms_all, host_s = {}, {}, {}

    def timed(name, fn):
        out, ms[name], ms_all[name] = mesh_rate._median_ms(fn, a.reps)
        return out

    def hosted(name, fn):
        out, host_s[name] = _once(fn)
        return out

    cl = timed('mesh_cluster', lambda: ops.mesh_cluster(dv, dc, cell, org))
    nc = int(cl.counts.shape[0])
    quadrics, inc = timed('mesh_cluster_quadrics', lambda: ops.mesh_cluster_quadrics(dv, df, cl.vertex_cluster, nc, cell, org))
    placed = {p: timed('mesh_cluster_place_' + p, lambda p=p: ops.mesh_cluster_place(cl.cells, cl.counts, cl.position_sums, cl.color_sums,
                                                                                     quadrics, cell, org, p)) for p in ('mean', 'quadric')}
    move = timed('mesh_cluster_max_move', lambda: ops.mesh_cluster_max_move(dv, cl.vertex_cluster, placed['quadric'][0]))
    rewritten, keep, drops = timed('mesh_cluster_faces', lambda: ops.mesh_cluster_faces(df, cl.vertex_cluster))
    selected = timed('mesh_select', lambda: ops.mesh_select(placed['quadric'][0], placed['quadric'][1], rewritten, keep))
    whole, whole_s = {}, {}
    for p in ('mean', 'quadric'):
        simplify_mesh.simplify_device(dv, dc, df, cell, p, org)                       # the warm-up
        runs = [_once(lambda p=p: simplify_mesh.simplify_device(dv, dc, df, cell, p, org)) for _ in range(a.reps)]
        whole[p], whole_s[p] = runs[-1][0], [s for _, s in runs]
    # the restatement, on the same mesh
    want_cl = hosted('cluster', lambda: S.cluster(vertices, colors, cell, org))
    want_q, want_inc = hosted('quadrics', lambda: S.quadrics(vertices, faces, want_cl['vertex_cluster'], nc, cell, org))
    want_pl = {p: hosted('place_' + p, lambda p=p: S.place(want_cl['cells'], want_cl['counts'], want_cl['position_sums'], want_cl['color_sums'],
                                                           want_q, cell, org, p)) for p in ('mean', 'quadric')}
    want_move = hosted('max_move', lambda: S.max_move(vertices, want_cl['vertex_cluster'], want_pl['quadric']['positions']))
    want_rw = hosted('rewrite_faces', lambda: S.rewrite_faces(faces, want_cl['vertex_cluster']))
    want_sel = hosted('select', lambda: T.select(want_pl['quadric']['positions'], want_pl['quadric']['colors'], want_rw['faces'], want_rw['keep']))
    host_s['whole_quadric'] = sum(host_s[k] for k in ('cluster', 'quadrics', 'place_quadric', 'max_move', 'rewrite_faces', 'select'))
    host_s['whole_mean'] = sum(host_s[k] for k in ('cluster', 'place_mean', 'max_move', 'rewrite_faces', 'select'))
    same = lambda g, w: np.array_equal(g.cpu().numpy().view(np.uint8), np.ascontiguousarray(w).view(np.uint8))          # noqa: E731
    assert all(same(getattr(cl, k), want_cl[k]) for k in ('vertex_cluster', 'cells', 'counts', 'position_sums', 'color_sums'))
    differing = int((quadrics.cpu().numpy() != want_q).sum())
    assert same(inc, want_inc) and (np.abs(quadrics.cpu().numpy() - want_q) <= want_inc[:, None]).all()
    assert same(placed['mean'][0], want_pl['mean']['positions']) and same(placed['mean'][1], want_pl['mean']['colors'])
    sure = want_pl['quadric']['margin'] >= 1e-6
    position_error = float(np.abs(placed['quadric'][0].cpu().numpy().astype(np.float64)
                                  - want_pl['quadric']['positions'].astype(np.float64))[sure].max())
    placed_differ = int((placed['quadric'][2].cpu().numpy() != want_pl['quadric']['placed'])[sure].sum())
    assert same(rewritten, want_rw['faces']) and same(keep, want_rw['keep'])
    assert drops == {k: want_rw[k] for k in drops} and same(selected[2], want_sel[2]) and len(selected[0]) == len(want_sel[0])
    report = {p: {k: v for k, v in whole[p][3].items()} for p in whole}
    # what the two placements do to a sphere: the radius of the output vertices
    radius = {p: np.linalg.norm(whole[p][0].cpu().numpy().astype(np.float64), axis=1) for p in whole}
    radius['input'] = np.linalg.norm(vertices.astype(np.float64), axis=1)
    shape = {p: {'mean_radius_error': float(r.mean() - mesh_rate.RADIUS), 'rms_radius_error': float(np.sqrt(((r - mesh_rate.RADIUS) ** 2).mean())),
                 'max_radius_error': float(np.abs(r - mesh_rate.RADIUS).max())} for p, r in radius.items()}
    return {'device': torch.cuda.get_device_name(dev), 'vertices': nv, 'faces': nf, 'cell': cell, 'cell_voxels': a.cell_voxels, 'origin': list(org),
            'clusters': nc, 'ms': ms, 'ms_all': ms_all, 'host_s': host_s, 'simplify_device_s': {p: float(np.median(s)) for p, s in whole_s.items()},
            'simplify_device_s_all': whole_s, 'report': report, 'quadric_words_differing': differing, 'low_margin_clusters': int((~sure).sum()),
            'largest_position_difference': position_error, 'placed_differ': placed_differ, 'max_move': move, 'restated_max_move': want_move,
            'sphere': shape, 'faces_per_s_quadrics': nf / (ms['mesh_cluster_quadrics'] * 1e-3),
            'faces_per_s_faces': nf / (ms['mesh_cluster_faces'] * 1e-3), 'vertices_per_s_cluster': nv / (ms['mesh_cluster'] * 1e-3),
            'stages_ms_quadric': sum(ms[k] for k in ('mesh_cluster', 'mesh_cluster_quadrics', 'mesh_cluster_place_quadric',
                                                     'mesh_cluster_max_move', 'mesh_cluster_faces', 'mesh_select')),
            'speedup_over_restatement_quadric': host_s['whole_quadric'] / (1e-3 * sum(
                ms[k] for k in ('mesh_cluster', 'mesh_cluster_quadrics', 'mesh_cluster_place_quadric', 'mesh_cluster_max_move',
                                'mesh_cluster_faces', 'mesh_select')))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--rows', type=int, default=296)
    ap.add_argument('--cols', type=int, default=400)
    ap.add_argument('--voxel', type=float, default=0.006)
    ap.add_argument('--min_weight', type=float, default=2.0)
    ap.add_argument('--max_blocks', type=int, default=131072)
    ap.add_argument('--cell_voxels', type=float, default=4.0)
    ap.add_argument('--reps', type=int, default=5)
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
                         'sphere_radius': mesh_rate.RADIUS, 'cell_voxels': a.cell_voxels, 'cameras': 'tests/scan_render_restated.ring_cameras'},
               'reps': a.reps}
    common = [x for k in ('maps', 'rows', 'cols', 'voxel', 'min_weight', 'max_blocks', 'cell_voxels', 'reps') for x in ('--' + k, str(getattr(a, k)))]
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:                        # a step that fails or runs out of time ends the run
            part = os.path.join(tmp, step + '.json')
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--out', part] + common, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print('mesh_simplify_rate: step %s ended with %d: nothing further is run' % (step, rc), file=sys.stderr)
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
