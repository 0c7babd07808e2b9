"""Mesh smoothing rates (csrc/mesh_smooth.hip, ops/mesh_smooth.py) beside the numpy restatement.

The mesh is tools_dev/mesh_rate.py's: the analytic sphere in --maps (64) ring cameras of --rows x --cols (296 x 400), voxel --voxel
(0.006), meshed by ops.tsdf_integrate and ops.tsdf_mesh: about 2.3 M faces.

    kernels   HIP events around atvs_mesh_adjacency (the whole build: table, degree walk, scan, scatter), one atvs_mesh_smooth_pass,
              ten Taubin iterations (twenty passes ping-ponging two q buffers) and the normals (atvs_mesh_face_extent,
              atvs_mesh_vertex_normal_sums, atvs_mesh_vertex_normals), each on buffers made beforehand; medians of --reps (9) after
              a warm-up, every run kept.  On the same mesh in the same process, wall clock on one host thread, once: the same four
              of tests/mesh_smooth_restated.py.  The device's adjacency, q after the ten iterations and normal sums are compared
              with the host's.  Effective bandwidth of a pass counts the 24 bytes of q_in gathered per neighbour entry, the
              neighbour index, and per vertex degree, flags, offset, q_in and q_out.

The step runs as a child process under its own time limit; a step that fails ends the run.

    python tools_dev/mesh_smooth_rate.py --out profiles/mesh_smooth.json
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
import mesh_smooth_restated as R  # noqa: E402
import mesh_rate  # noqa: E402
from fusion_rate import measured_head  # noqa: E402

STEPS = (('kernels', 900),)
MEASURED = ('a-tvsnet_amd/csrc/mesh_smooth.hip', 'a-tvsnet_amd/csrc/cloud_scan.h', 'a-tvsnet_amd/ops/mesh_smooth.py')
ITERATIONS, LAM, MU = 10, 0.5, -0.53


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
    torch.set_num_threads(1)
    cams, depths, images, trunc, origin, dims = mesh_rate.scene(a)
    d, c, im = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams, images))
    volume = ops.tsdf_integrate(d, c, a.voxel, trunc, origin, dims, images=im, max_blocks=a.max_blocks)
    dv, _, df = (t.contiguous() for t in ops.tsdf_mesh(volume, a.min_weight))
    vertices, faces = dv.cpu().numpy(), df.cpu().numpy()
    nv, nf = len(vertices), len(faces)
    ms, ms_all, host_s, spread = {}, {}, {}, {}

    def timed(name, fn):
        out, _, times = mesh_rate._median_ms(fn, a.reps)
        ms_all[name] = list(times)
        ms[name] = float(np.median(times))
        spread[name] = [float(min(times)), float(max(times))]
        return out

    def hosted(name, fn):
        out, host_s[name] = _once(fn)
        return out

    degree, flags = (torch.empty(nv, dtype=torch.int32, device=dev) for _ in range(2))
    offsets = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    neighbours = torch.empty(6 * nf, dtype=torch.int32, device=dev)
    scratch = torch.empty(_size('atvs_mesh_adjacency_scratch_size', nv, nf), dtype=torch.uint8, device=dev)
    words = torch.empty(7, dtype=torch.int64, device=dev)
    timed('adjacency', lambda: _call('atvs_mesh_adjacency', _p(dv), nv, _p(df), nf, _p(scratch), scratch.numel(), _p(degree), _p(flags),
                                     _p(offsets), _p(neighbours), _p(words), _stream()))
    info = dict(zip(ops.MESH_ADJACENCY_INFO, (int(x) for x in words.cpu().tolist())))
    entries = 2 * info['pairs']
    org, step = R.lattice(vertices)
    q0, _ = ops.mesh_quantize(dv, org, step)
    qa, qb = torch.empty_like(q0), torch.empty_like(q0)
    tallies = torch.zeros(2, dtype=torch.int32, device=dev)

    def one_pass(src, dst, factor):
        _call('atvs_mesh_smooth_pass', _p(src), nv, _p(degree), _p(flags), _p(offsets), _p(neighbours), entries, factor, 0, _p(dst), _p(tallies),
              _stream())

    def taubin():
        src = q0
        for k in range(ITERATIONS):
            one_pass(src, qa, LAM)
            one_pass(qa, qb, MU)
            src = qb
        return qb
    timed('pass', lambda: one_pass(q0, qa, LAM))
    q_end = timed('taubin_10', taubin)
    assert tallies.cpu().tolist() == [0, 0]
    ewords = torch.empty(4, dtype=torch.int64, device=dev)
    sums = torch.empty((nv, 3), dtype=torch.int64, device=dev)
    incidences = torch.empty(nv, dtype=torch.int32, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    normals = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    unit = a.voxel * a.voxel

    def all_normals():
        _call('atvs_mesh_face_extent', _p(dv), nv, _p(df), nf, _p(ewords), _stream())
        _call('atvs_mesh_vertex_normal_sums', _p(dv), nv, _p(df), nf, unit, _p(sums), _p(incidences), _p(bad), _stream())
        _call('atvs_mesh_vertex_normals', _p(sums), nv, _p(normals), _stream())
    timed('normals', all_normals)
    timed('face_extent', lambda: _call('atvs_mesh_face_extent', _p(dv), nv, _p(df), nf, _p(ewords), _stream()))
    timed('normal_sums', lambda: _call('atvs_mesh_vertex_normal_sums', _p(dv), nv, _p(df), nf, unit, _p(sums), _p(incidences), _p(bad), _stream()))
    timed('normals_from_sums', lambda: _call('atvs_mesh_vertex_normals', _p(sums), nv, _p(normals), _stream()))
    whole = timed('mesh_smooth', lambda: ops.mesh_smooth(dv, df, ITERATIONS, LAM, MU))
    # the restatement, on the same mesh
    adj = hosted('adjacency', lambda: R.adjacency(vertices, faces))
    assert adj['info'] == info
    for key, t in (('degree', degree), ('flags', flags), ('offsets', offsets)):
        assert np.array_equal(t.cpu().numpy(), adj[key]), key
    hq0, _ = R.quantize(vertices, org, step)
    hosted('pass', lambda: R.smooth_pass(hq0, adj, LAM))

    def host_taubin():
        q = hq0
        for _ in range(ITERATIONS):
            q, _c = R.smooth_pass(q, adj, LAM)
            q, _c = R.smooth_pass(q, adj, MU)
        return q
    hq = hosted('taubin_10', host_taubin)
    assert np.array_equal(q_end.cpu().numpy(), hq)
    assert np.array_equal(whole[0].cpu().numpy().view(np.uint32), R.dequantize(hq, hq0, vertices, org, step).view(np.uint32))

    def host_normals():
        R.face_extent(vertices, faces)
        s, i = R.vertex_normal_sums(vertices, faces, unit)
        return s, i, R.normals_from_sums(s)
    hs, hi, hn = hosted('normals', host_normals)
    diff = np.abs(sums.cpu().numpy() - hs)
    assert np.array_equal(incidences.cpu().numpy(), hi) and (diff <= hi[:, None]).all()
    pass_bytes = entries * (24 + 4) + nv * (4 + 4 + 4 + 24 + 24)
    before, after = (np.linalg.norm(x.astype(np.float64), axis=1) for x in (vertices, whole[0].cpu().numpy()))
    return {'device': torch.cuda.get_device_name(dev), 'vertices': nv, 'faces': nf, 'adjacency': info, 'neighbour_entries': entries,
            'mean_degree': entries / float(max(nv, 1)), 'max_degree': int(adj['degree'].max(initial=0)), 'iterations': ITERATIONS, 'lam': LAM, 'mu': MU,
            'step': step, 'normal_area_unit': unit, 'ms': ms, 'ms_min_max': spread, 'ms_all': ms_all, 'host_s': host_s,
            'speedup_over_restatement': {k: host_s[k] / (ms[k] * 1e-3) for k in host_s},
            'faces_per_s_adjacency': nf / (ms['adjacency'] * 1e-3), 'vertices_per_s_pass': nv / (ms['pass'] * 1e-3),
            'pass_bytes': pass_bytes, 'pass_gb_per_s': pass_bytes / (ms['pass'] * 1e-3) / 1e9,
            'faces_per_s_normals': nf / (ms['normals'] * 1e-3), 'normal_sum_words_that_differ': int((diff != 0).sum()),
            'sphere': {'radius_std_before': float(before.std()), 'radius_std_after': float(after.std()),
                       'mean_radius_before': float(before.mean()), 'mean_radius_after': float(after.mean())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--rows', type=int, default=296)
    ap.add_argument('--cols', type=int, default=400)
    ap.add_argument('--voxel', type=float, default=0.006)
    ap.add_argument('--min_weight', type=float, default=2.0)
    ap.add_argument('--max_blocks', type=int, default=131072)
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
                         'sphere_radius': mesh_rate.RADIUS, 'cameras': 'tests/scan_render_restated.ring_cameras'},
               'reps': a.reps}
    common = [x for k in ('maps', 'rows', 'cols', 'voxel', 'min_weight', 'max_blocks', 'reps') for x in ('--' + k, str(getattr(a, k)))]
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in STEPS:                        # a step that fails or runs out of time ends the run
            part = os.path.join(tmp, step + '.json')
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--out', part] + common, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print('mesh_smooth_rate: step %s ended with %d: nothing further is run' % (step, rc), file=sys.stderr)
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
