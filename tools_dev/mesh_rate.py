"""TSDF fusion and marching-tetrahedra rates (csrc/tsdf.hip, atvsnet/mesh_fusion.py) beside the numpy restatement.

The scene: the sphere of tests/tsdf_restated.py (radius 0.9) rendered analytically into --maps (64) ring cameras of --rows x --cols
(296 x 400, the size DESIGN.md section 10.2 quotes), voxel --voxel (0.006, about a pixel's footprint on the surface), trunc 4 voxels.

    kernels      HIP events around each entry point of ops.tsdf_integrate and ops.tsdf_mesh, medians of --reps after a warm-up:
                 mark, the directory scan, assign (coordinates + view masks), integrate, the any-weight scan + gather; mesh_count,
                 the two scans, mesh_emit.  With them the counts: marked and kept blocks, voxel-views, vertices, faces.
    scene        mesh_fusion.SceneMesh end to end on a depth_fusion.SceneFusion staged with the same maps: wall clock of run()
                 (the fusion's own run() apart), and its report.
    restatement  tests/tsdf_restated.py on the host: integrate over a sub-box of --host_blocks^3 blocks and --host_views views, mesh
                 of that sub-box, as voxel-views / s and faces / s.  The whole scene is not restated: 64 Mi voxels x 64 views.

    carve        (--carve, a run of its own) free-space carving on the same scene: integrate without and with carving on the same
                 slots, the free-view launch, the free mask's bits out of slots x views, the voxels with a free vote.

    weighted     (--weights, alias --support, a run of its own) the consistency mask and the view weights on the same scene:
                 atvs_fusion_support beside atvs_fusibile_scene (count, scan and scatter: the count pass has no entry point of its
                 own) on the same slab, and the integrate kernel's plain, carving and weighted forms on the same slots, the old
                 forms twice, alternating.  --baseline runs the old forms alone: the step a checkout of the parent commit can run.

Each step runs as a child process under its own time limit, one after the other; the first that fails ends the run.

    python tools_dev/mesh_rate.py --out profiles/tsdf_mesh.json
    python tools_dev/mesh_rate.py --carve --out profiles/tsdf_mesh_carve.json
    python tools_dev/mesh_rate.py --weights --out profiles/tsdf_mesh_weighted.json
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
import tsdf_restated as R  # noqa: E402
from scan_render_restated import ring_cameras  # noqa: E402
from fusion_rate import measured_head  # noqa: E402

RADIUS = 0.9
STEPS = (('kernels', 300), ('scene', 300), ('restatement', 400))
CARVE_STEPS = (('carve', 300),)
WEIGHTED_STEPS = (('weighted', 300),)
BASELINE_STEPS = (('baseline', 300),)
MEASURED = ('a-tvsnet_amd/csrc/tsdf.hip', 'a-tvsnet_amd/csrc/fusion_support.hip', 'a-tvsnet_amd/csrc/fusion_pixel.h',
            'a-tvsnet_amd/csrc/scan_project.h', 'a-tvsnet_amd/csrc/cloud_scan.h', 'a-tvsnet_amd/ops/tsdf.py',
            'a-tvsnet_amd/atvsnet/mesh_fusion.py')


def sources_sha1():
    import hashlib
    h = hashlib.sha1()
    for p in MEASURED:
        with open(os.path.join(ROOT, p), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def scene(a):
    cams = ring_cameras(a.maps, a.rows, a.cols)
    depths, images = R.sphere_depths(cams, a.rows, a.cols, RADIUS)
    trunc = 4.0 * a.voxel
    pad = trunc + 8.0 * a.voxel
    origin = np.full(3, -RADIUS - pad) + np.array([0.0013, 0.0007, 0.0021])          # not a round number
    dims = tuple(int(np.ceil((RADIUS + pad - o) / (8.0 * a.voxel))) for o in origin)
    return cams, depths, images, trunc, origin, dims


def _median_ms(fn, reps):
    import torch
    out, times = fn(), []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return out, float(np.median(times)), times


def step_kernels(a):
    """The entry points one by one, as ops.tsdf_integrate and ops.tsdf_mesh call them."""
    import torch
    from atvsnet_amd import ops
    from atvsnet_amd.ops import tsdf as T
    from atvsnet_amd.ops.base import _call, _p, _stream
    from atvsnet_amd.ops.cloud import _vec3
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = scene(a)
    d, c, im = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams, images))
    n, rows, cols = depths.shape
    bx, by, bz = dims
    nbk = bx * by * bz
    box = (a.voxel, trunc, _vec3(origin, 'origin'), bx, by, bz, 0.0)
    directory = torch.empty(nbk, dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    ms, all_ms = {}, {}

    def timed(name, fn):
        out, ms[name], all_ms[name] = _median_ms(fn, a.reps)
        return out

    timed('mark', lambda: _call('atvs_tsdf_mark', _p(d), _p(c), n, rows, cols, *box, _p(directory), _p(err), _stream()))
    marks = directory.clone()

    def scan_directory():
        directory.copy_(marks)
        return T._scan(directory, nbk)
    timed('directory_copy_and_scan', scan_directory)
    count = int(T._scan(directory.copy_(marks), nbk).item())
    assert int(err.item()) == 0 and 0 < count <= a.max_blocks, count
    words = (n + 63) // 64
    coords = torch.empty((count, 3), dtype=torch.int32, device=dev)
    masks = torch.empty((count, words), dtype=torch.int64, device=dev)
    timed('assign', lambda: _call('atvs_tsdf_assign', _p(d), _p(c), n, rows, cols, *box, _p(directory), count, _p(coords), _p(masks),
                                  _p(err), _stream()))
    tsdf = torch.empty((count, 8, 8, 8), dtype=torch.float32, device=dev)
    weight = torch.empty_like(tsdf)
    color = torch.empty((count, 8, 8, 8, 3), dtype=torch.float32, device=dev)
    keep = torch.empty(count, dtype=torch.int32, device=dev)
    timed('integrate', lambda: _call('atvs_tsdf_integrate', _p(d), _p(im), 3, _p(c), n, rows, cols, *box, _p(coords), _p(masks), count,
                                     _p(tsdf), _p(weight), _p(color), _p(keep), _stream()))
    bits = masks.cpu().numpy().view(np.uint64)
    block_views = int(sum(bin(int(w)).count('1') for w in bits.reshape(-1)))
    volume, ms['tsdf_integrate_call'], all_ms['tsdf_integrate_call'] = _median_ms(
        lambda: ops.tsdf_integrate(d, c, a.voxel, trunc, origin, dims, images=im, max_blocks=a.max_blocks), a.reps)
    nb = volume.num_blocks
    cube_ok = torch.empty(nb * 512, dtype=torch.uint8, device=dev)
    emask = torch.empty(nb * 512, dtype=torch.uint8, device=dev)
    counts = torch.empty((2, nb * 512), dtype=torch.int32, device=dev)
    timed('mesh_count', lambda: _call('atvs_tsdf_mesh_count', _p(volume.blocks), nb, bx, by, bz, _p(volume.tsdf), _p(volume.weight),
                                      a.min_weight, _p(cube_ok), _p(emask), _p(counts[0]), _p(counts[1]), _stream()))
    raw = counts.clone()
    totals = torch.empty(2, dtype=torch.int64, device=dev)

    def scans():
        counts.copy_(raw)
        T._scan(counts[0], nb * 512, totals[0:1])
        T._scan(counts[1], nb * 512, totals[1:2])
    timed('mesh_copy_and_scans', scans)
    nv, nf = (int(v) for v in totals.cpu())
    vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((nv, 3), dtype=torch.uint8, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    timed('mesh_emit', lambda: _call('atvs_tsdf_mesh_emit', _p(volume.blocks), nb, bx, by, bz, a.voxel, box[2], _p(volume.tsdf),
                                     _p(volume.color), _p(emask), _p(counts[0]), _p(counts[1]), nv, nf, _p(vertices), _p(colors),
                                     _p(faces), _stream()))
    mesh, ms['tsdf_mesh_call'], all_ms['tsdf_mesh_call'] = _median_ms(lambda: ops.tsdf_mesh(volume, a.min_weight), a.reps)
    assert torch.equal(mesh[0], vertices) and torch.equal(mesh[2], faces)
    voxel_views = block_views * 512
    return {'device': torch.cuda.get_device_name(dev), 'dims': list(dims), 'directory_blocks': nbk, 'marked_blocks': count, 'kept_blocks': nb,
            'block_views': block_views, 'voxel_views': voxel_views, 'valid_voxels': int((volume.weight >= a.min_weight).sum().item()),
            'vertices': nv, 'faces': nf, 'ms': ms, 'ms_all': all_ms,
            'integrate_voxel_views_per_s': voxel_views / (ms['integrate'] * 1e-3),
            'integrate_gather_bytes_per_voxel_view': 16, 'integrate_gather_GBps': 16.0 * voxel_views / (ms['integrate'] * 1e-3) / 1e9,
            'extract_faces_per_s': nf / ((ms['mesh_count'] + ms['mesh_copy_and_scans'] + ms['mesh_emit']) * 1e-3)}


def step_carve(a):
    """Integration with and without carving on the slots ops.tsdf_integrate would make, entry point by entry point."""
    import torch
    from atvsnet_amd import ops
    from atvsnet_amd.ops import tsdf as T
    from atvsnet_amd.ops.base import _call, _p, _stream
    from atvsnet_amd.ops.cloud import _vec3
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = scene(a)
    d, c, im = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams, images))
    n, rows, cols = depths.shape
    bx, by, bz = dims
    nbk = bx * by * bz
    org = _vec3(origin, 'origin')
    box = (a.voxel, trunc, org, bx, by, bz, 0.0)
    directory = torch.empty(nbk, dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    _call('atvs_tsdf_mark', _p(d), _p(c), n, rows, cols, *box, _p(directory), _p(err), _stream())
    count = int(T._scan(directory, nbk).item())
    assert int(err.item()) == 0 and 0 < count <= a.max_blocks, count
    words = (n + 63) // 64
    coords = torch.empty((count, 3), dtype=torch.int32, device=dev)
    masks = torch.empty((count, words), dtype=torch.int64, device=dev)
    free_masks = torch.empty((count, words), dtype=torch.int64, device=dev)
    _call('atvs_tsdf_assign', _p(d), _p(c), n, rows, cols, *box, _p(directory), count, _p(coords), _p(masks), _p(err), _stream())
    tsdf = torch.empty((count, 8, 8, 8), dtype=torch.float32, device=dev)
    weight, free = torch.empty_like(tsdf), torch.empty_like(tsdf)
    color = torch.empty((count, 8, 8, 8, 3), dtype=torch.float32, device=dev)
    keep = torch.empty(count, dtype=torch.int32, device=dev)
    ms, all_ms = {}, {}

    def timed(name, fn):
        out, ms[name], all_ms[name] = _median_ms(fn, a.reps)
        return out

    timed('integrate', lambda: _call('atvs_tsdf_integrate', _p(d), _p(im), 3, _p(c), n, rows, cols, *box, _p(coords), _p(masks), count,
                                     _p(tsdf), _p(weight), _p(color), _p(keep), _stream()))
    plain_tsdf, plain_weight = tsdf.clone(), weight.clone()
    timed('free_views', lambda: _call('atvs_tsdf_free_views', _p(coords), count, _p(c), n, rows, cols, a.voxel, org, bx, by, bz, 0.0,
                                      _p(free_masks), _stream()))
    timed('integrate_carve', lambda: _call('atvs_tsdf_integrate_carve', _p(d), _p(im), 3, _p(c), n, rows, cols, *box, _p(coords), _p(masks),
                                           _p(free_masks), a.carve_weight, count, _p(tsdf), _p(weight), _p(color), _p(free), _p(keep),
                                           _stream()))
    assert torch.equal(weight, plain_weight)

    def popcount(m):
        return int(sum(bin(int(w)).count('1') for w in m.cpu().numpy().view(np.uint64).reshape(-1)))
    band_bits, loop_bits = popcount(masks), popcount(masks | free_masks)
    free_bits = popcount(free_masks)
    _, ms['tsdf_integrate_call'], all_ms['tsdf_integrate_call'] = _median_ms(
        lambda: ops.tsdf_integrate(d, c, a.voxel, trunc, origin, dims, images=im, max_blocks=a.max_blocks), a.reps)
    volume, ms['tsdf_integrate_call_carve'], all_ms['tsdf_integrate_call_carve'] = _median_ms(
        lambda: ops.tsdf_integrate(d, c, a.voxel, trunc, origin, dims, images=im, max_blocks=a.max_blocks, carve_weight=a.carve_weight), a.reps)
    valid = volume.weight >= a.min_weight
    flipped = int(((tsdf < 0) != (plain_tsdf < 0))[plain_weight >= a.min_weight].sum().item())
    return {'device': torch.cuda.get_device_name(dev), 'carve_weight': a.carve_weight, 'marked_blocks': count, 'kept_blocks': volume.num_blocks,
            'views': n, 'band_mask_bits': band_bits, 'free_mask_bits': free_bits, 'loop_mask_bits': loop_bits,
            'free_mask_share_of_slots_x_views': free_bits / float(count * n), 'voxel_views_plain': band_bits * 512,
            'voxel_views_carve': loop_bits * 512, 'valid_voxels': int(valid.sum().item()),
            'free_voxels': int((valid & (volume.free > 0)).sum().item()), 'max_free': float(volume.free.max().item()),
            'valid_voxels_whose_sign_flipped': flipped, 'ms': ms, 'ms_all': all_ms,
            'carve_voxel_views_per_s': loop_bits * 512 / (ms['integrate_carve'] * 1e-3)}


def step_weighted(a):
    """The support kernel beside atvs_fusibile_scene on the same slab, and the three forms of the integrate kernel on the same slots:
    plain, carving, weighted without and with carving (the weights are the support kernel's)."""
    import torch
    from atvsnet_amd.atvsnet import depth_fusion as DF
    from atvsnet_amd.ops import tsdf as T
    from atvsnet_amd.ops.base import _call, _p, _size, _stream
    from atvsnet_amd.ops.cloud import _vec3
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = scene(a)
    d, c, im = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams, images))
    n, rows, cols = depths.shape
    ms, all_ms = {}, {}

    def timed(name, fn):
        out, ms[name], all_ms[name] = _median_ms(fn, a.reps)
        return out

    # the slab the fusion would hold: the fake normal where there is a depth, the images as float4
    Ps = [np.array([[k[12], 0, k[14]], [0, k[13], k[15]], [0, 0, 1.0]]) @ np.concatenate([k[:9].reshape(3, 3), k[9:12].reshape(3, 1)], 1) for k in cams]
    cams28 = torch.from_numpy(DF.pack_cameras(Ps)).to(dev)
    fake = torch.where(d > 0, torch.full_like(d, float(np.float32(1.0) / np.float32(1.732050808))), torch.zeros_like(d))
    nd = torch.stack([fake, fake, fake, d], dim=-1).contiguous()
    img4 = torch.cat([im, torch.zeros_like(im[..., :1])], dim=-1).contiguous()
    disp, ang, ncons = 0.01, DF.NORMAL_THRESHOLD, 2
    count = torch.empty((n, rows, cols), dtype=torch.int32, device=dev)
    masked, wplane = torch.empty_like(d), torch.empty_like(d)
    timed('support_all_outputs', lambda: _call('atvs_fusion_support', _p(cams28), _p(nd), n, rows, cols, disp, ang, ncons, _p(count), _p(masked),
                                               _p(wplane), _stream()))
    timed('support_count_alone', lambda: _call('atvs_fusion_support', _p(cams28), _p(nd), n, rows, cols, disp, ang, ncons, _p(count), None, None,
                                               _stream()))
    capacity = n * rows * cols
    scratch = torch.empty(_size('atvs_fusibile_scene_scratch_size', n, rows, cols), dtype=torch.uint8, device=dev)
    points = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((capacity, 3), dtype=torch.uint8, device=dev)
    n_points = torch.empty(1, dtype=torch.int32, device=dev)
    timed('fusibile_scene_count_scan_scatter', lambda: _call('atvs_fusibile_scene', _p(cams28), _p(nd), _p(img4), n, rows, cols, disp, ang, ncons,
                                                             _p(scratch), scratch.numel(), _p(points), _p(colors), capacity, _p(n_points),
                                                             _stream()))
    fused_points = int(n_points.item())                  # beside samples_kept: the fusion also keeps a created pixel without a depth

    bx, by, bz = dims
    nbk = bx * by * bz
    org = _vec3(origin, 'origin')
    box = (a.voxel, trunc, org, bx, by, bz, 0.0)
    directory = torch.empty(nbk, dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    _call('atvs_tsdf_mark', _p(d), _p(c), n, rows, cols, *box, _p(directory), _p(err), _stream())
    slots = int(T._scan(directory, nbk).item())
    assert int(err.item()) == 0 and 0 < slots <= a.max_blocks, slots
    words = (n + 63) // 64
    coords = torch.empty((slots, 3), dtype=torch.int32, device=dev)
    masks = torch.empty((slots, words), dtype=torch.int64, device=dev)
    free_masks = torch.empty((slots, words), dtype=torch.int64, device=dev)
    _call('atvs_tsdf_assign', _p(d), _p(c), n, rows, cols, *box, _p(directory), slots, _p(coords), _p(masks), _p(err), _stream())
    _call('atvs_tsdf_free_views', _p(coords), slots, _p(c), n, rows, cols, a.voxel, org, bx, by, bz, 0.0, _p(free_masks), _stream())
    tsdf = torch.empty((slots, 8, 8, 8), dtype=torch.float32, device=dev)
    weight, free = torch.empty_like(tsdf), torch.empty_like(tsdf)
    color = torch.empty((slots, 8, 8, 8, 3), dtype=torch.float32, device=dev)
    keep = torch.empty(slots, dtype=torch.int32, device=dev)
    ones = torch.ones_like(d)

    def plain():
        _call('atvs_tsdf_integrate', _p(d), _p(im), 3, _p(c), n, rows, cols, *box, _p(coords), _p(masks), slots, _p(tsdf), _p(weight), _p(color),
              _p(keep), _stream())

    def carve():
        _call('atvs_tsdf_integrate_carve', _p(d), _p(im), 3, _p(c), n, rows, cols, *box, _p(coords), _p(masks), _p(free_masks), a.carve_weight,
              slots, _p(tsdf), _p(weight), _p(color), _p(free), _p(keep), _stream())

    def weighted(w, carving):
        _call('atvs_tsdf_integrate_weighted', _p(d), _p(w), _p(im), 3, _p(c), n, rows, cols, *box, _p(coords), _p(masks),
              _p(free_masks) if carving else None, a.carve_weight, slots, _p(tsdf), _p(weight), _p(color), _p(free) if carving else None,
              _p(keep), _stream())

    # the old forms twice, alternating with the new one: what a baseline at the parent commit is compared with
    for tag in ('', '_again'):
        timed('integrate' + tag, plain)
        timed('integrate_carve' + tag, carve)
        timed('integrate_weighted' + tag, lambda: weighted(wplane, False))
        timed('integrate_weighted_carve' + tag, lambda: weighted(wplane, True))
    plain()
    ref = (tsdf.clone(), weight.clone(), color.clone())
    weighted(ones, False)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ref, (tsdf, weight, color)))      # all-ones: the same bits
    bits = int(sum(bin(int(w)).count('1') for w in masks.cpu().numpy().view(np.uint64).reshape(-1)))
    return {'device': torch.cuda.get_device_name(dev), 'views': n, 'pixels': capacity, 'disp_threshold': disp, 'num_consistent': ncons,
            'samples': int((d > 0).sum().item()), 'samples_kept': int((masked > 0).sum().item()), 'fused_points': fused_points,
            'pixels_without_depth_with_count_ge_num_consistent': int(((d <= 0) & (count >= ncons)).sum().item()), 'marked_blocks': slots,
            'voxel_views_plain': bits * 512, 'ms': ms, 'ms_all': all_ms,
            'support_over_fusibile_scene': ms['support_all_outputs'] / ms['fusibile_scene_count_scan_scatter'],
            'weighted_over_plain': ms['integrate_weighted'] / ms['integrate'],
            'weighted_carve_over_carve': ms['integrate_weighted_carve'] / ms['integrate_carve']}


def step_baseline(a):
    """The plain and the carving form alone, on the same slots: the step that also runs on a checkout of the parent commit."""
    import torch
    from atvsnet_amd.ops import tsdf as T
    from atvsnet_amd.ops.base import _call, _p, _stream
    from atvsnet_amd.ops.cloud import _vec3
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = scene(a)
    d, c, im = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depths, cams, images))
    n, rows, cols = depths.shape
    bx, by, bz = dims
    nbk = bx * by * bz
    org = _vec3(origin, 'origin')
    box = (a.voxel, trunc, org, bx, by, bz, 0.0)
    directory = torch.empty(nbk, dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    _call('atvs_tsdf_mark', _p(d), _p(c), n, rows, cols, *box, _p(directory), _p(err), _stream())
    slots = int(T._scan(directory, nbk).item())
    words = (n + 63) // 64
    coords = torch.empty((slots, 3), dtype=torch.int32, device=dev)
    masks = torch.empty((slots, words), dtype=torch.int64, device=dev)
    free_masks = torch.empty((slots, words), dtype=torch.int64, device=dev)
    _call('atvs_tsdf_assign', _p(d), _p(c), n, rows, cols, *box, _p(directory), slots, _p(coords), _p(masks), _p(err), _stream())
    _call('atvs_tsdf_free_views', _p(coords), slots, _p(c), n, rows, cols, a.voxel, org, bx, by, bz, 0.0, _p(free_masks), _stream())
    tsdf = torch.empty((slots, 8, 8, 8), dtype=torch.float32, device=dev)
    weight, free = torch.empty_like(tsdf), torch.empty_like(tsdf)
    color = torch.empty((slots, 8, 8, 8, 3), dtype=torch.float32, device=dev)
    keep = torch.empty(slots, dtype=torch.int32, device=dev)
    ms, all_ms = {}, {}
    for tag in ('', '_again'):
        _, ms['integrate' + tag], all_ms['integrate' + tag] = _median_ms(
            lambda: _call('atvs_tsdf_integrate', _p(d), _p(im), 3, _p(c), n, rows, cols, *box, _p(coords), _p(masks), slots, _p(tsdf), _p(weight),
                          _p(color), _p(keep), _stream()), a.reps)
        _, ms['integrate_carve' + tag], all_ms['integrate_carve' + tag] = _median_ms(
            lambda: _call('atvs_tsdf_integrate_carve', _p(d), _p(im), 3, _p(c), n, rows, cols, *box, _p(coords), _p(masks), _p(free_masks),
                          a.carve_weight, slots, _p(tsdf), _p(weight), _p(color), _p(free), _p(keep), _stream()), a.reps)
    return {'device': torch.cuda.get_device_name(dev), 'marked_blocks': slots, 'ms': ms, 'ms_all': all_ms}


def step_scene(a):
    import torch
    from atvsnet_amd.atvsnet import depth_fusion as DF, mesh_fusion
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cams, depths, images, trunc, origin, dims = scene(a)
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
    t0 = time.perf_counter()
    points, _ = fusion.run()
    torch.cuda.synchronize()
    fuse_s = time.perf_counter() - t0
    runs = []
    for _ in range(a.reps + 1):                          # the first is the warm-up
        scene_mesh = mesh_fusion.SceneMesh(fusion, cam44, a.voxel, 4.0, a.min_weight, a.max_blocks)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scene_mesh.run()
        runs.append(time.perf_counter() - t0)
    return {'fused_points': int(len(points)), 'fusion_run_s': fuse_s, 'scene_mesh_run_s': float(np.median(runs[1:])), 'scene_mesh_run_s_all': runs[1:],
            'warm_up_s': runs[0], 'report': scene_mesh.report()}


def step_restatement(a):
    cams, depths, images, trunc, origin, dims = scene(a)
    b = a.host_blocks
    # a sub-box that holds surface: around the point of the sphere nearest camera 0
    centre = -cams[0, :9].reshape(3, 3).T @ cams[0, 9:12]
    corner = centre / np.linalg.norm(centre) * RADIUS - 4.0 * b * a.voxel
    sub_origin = origin + np.floor((corner - origin) / (8 * a.voxel)) * 8 * a.voxel
    views = np.linspace(0, len(cams) - 1, a.host_views).astype(int)
    t0 = time.perf_counter()
    vol = R.integrate(depths[views], cams[views], a.voxel, trunc, sub_origin, (b, b, b), images[views])
    t1 = time.perf_counter()
    mesh = R.mesh(vol['tsdf'], vol['weight'], vol['color'], sub_origin, a.voxel, 1.0)
    t2 = time.perf_counter()
    voxel_views = (8 * b) ** 3 * len(views)
    return {'what': 'tests/tsdf_restated.py (numpy, one host thread)', 'blocks': [b, b, b], 'views': len(views), 'voxel_views': voxel_views,
            'integrate_s': t1 - t0, 'integrate_voxel_views_per_s': voxel_views / (t1 - t0), 'faces': int(len(mesh[2])), 'mesh_s': t2 - t1,
            'mesh_faces_per_s': len(mesh[2]) / (t2 - t1) if len(mesh[2]) else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--maps', type=int, default=64)
    ap.add_argument('--rows', type=int, default=296)
    ap.add_argument('--cols', type=int, default=400)
    ap.add_argument('--voxel', type=float, default=0.006)
    ap.add_argument('--min_weight', type=float, default=2.0)
    ap.add_argument('--max_blocks', type=int, default=131072)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host_blocks', type=int, default=8)
    ap.add_argument('--host_views', type=int, default=4)
    ap.add_argument('--carve_weight', type=float, default=1.0)
    ap.add_argument('--carve', action='store_true', help='run the carve step alone (for profiles/tsdf_mesh_carve.json)')
    ap.add_argument('--weights', '--support', dest='weights', action='store_true',
                    help='run the weighted step alone (for profiles/tsdf_mesh_weighted.json)')
    ap.add_argument('--baseline', action='store_true', help='run the baseline step alone: the plain and carving forms, as the parent commit has them')
    ap.add_argument('--step', default=None, choices=[s for s, _ in STEPS + CARVE_STEPS + WEIGHTED_STEPS + BASELINE_STEPS], help='run one step in this process and write its result to --out')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.step is not None:
        result = {'kernels': step_kernels, 'scene': step_scene, 'restatement': step_restatement, 'carve': step_carve,
                  'weighted': step_weighted, 'baseline': step_baseline}[a.step](a)
        print(json.dumps({k: v for k, v in result.items() if not k.endswith('_all')}), flush=True)
        if a.out:
            with open(a.out, 'w') as f:
                json.dump(result, f)
        return 0
    summary = {'parent_commit': measured_head(), 'sources_sha1': sources_sha1(),
               'scene': {'maps': a.maps, 'rows': a.rows, 'cols': a.cols, 'voxel': a.voxel, 'trunc_voxels': 4.0, 'min_weight': a.min_weight,
                         'sphere_radius': RADIUS, 'cameras': 'tests/scan_render_restated.ring_cameras'},
               'reps': a.reps}
    passed = [k for k in ('maps', 'rows', 'cols', 'voxel', 'min_weight', 'max_blocks', 'reps', 'host_blocks', 'host_views', 'carve_weight')]
    common = [x for k in passed for x in ('--' + k, str(getattr(a, k)))]
    with tempfile.TemporaryDirectory() as tmp:
        for step, limit in (CARVE_STEPS if a.carve else WEIGHTED_STEPS if a.weights else BASELINE_STEPS if a.baseline else STEPS):                        # one after the other: a step that fails or runs out of time ends the run
            part = os.path.join(tmp, step + '.json')
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step, '--out', part] + common, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print('mesh_rate: step %s ended with %d: nothing further is run' % (step, rc), file=sys.stderr)
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
