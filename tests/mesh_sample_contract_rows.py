"""The rows of ops/mesh_sample.py for the buffer contract, registered in tests/buffer_contract_rows.py's table on import: that
table must name every entry point of include/atvsnet_hip.h that writes through a pointer or takes scratch
(tests/test_buffer_contract_host.py), and these are the rows for atvs_mesh_sample_counts, atvs_mesh_sample_scratch_size,
atvs_mesh_sample_offsets and atvs_mesh_sample_place.  tests/test_mesh_sample_host.py (the builders, without a GPU) and
tests/test_gpu_mesh_sample_contract.py (the three guarded runs) import this module and run the rows; pytest imports every test
module before it runs a test, so the table is whole whenever the suite is collected."""
import collections

import numpy as np

import buffer_contract_rows as BR

SAMPLE_DENSITY, SAMPLE_SEED = 8.0, 5           # a face of BR._mesh spans up to a few units of area: tens of samples on the large ones
# one face of one vertex has no area and no sample: nothing to place there, and no entry point to reach
SAMPLE_SIZES = collections.OrderedDict((k, dict(v, entries=()) if v == {'V': 1, 'F': 1} else v) for k, v in BR.MESH_SIZES.items())
NAMES = ('mesh_sample_counts', 'mesh_sample_points')


def _sample_points_run(ops, d, place):
    counts = place(ops.mesh_sample_counts(d['vertices'], d['faces'], SAMPLE_DENSITY, SAMPLE_SEED)[0])
    return ops.mesh_sample_points(d['vertices'], d['colors'], d['faces'], counts, SAMPLE_SEED, normals=True)


if NAMES[0] not in BR.ROWS:                      # (imported under two names -- as a module and by a test -- it registers once)
    BR.Row('mesh_sample_counts', ('atvs_mesh_sample_counts',), BR.MESH_SIZES, BR._mesh, BR._mesh_shapes,
           run=lambda ops, d, place: ops.mesh_sample_counts(d['vertices'], d['faces'], SAMPLE_DENSITY, SAMPLE_SEED),
           select=lambda r: [r[0], r[1], BR._t([r[2][k] for k in sorted(r[2])], np.int64)], names=('counts', 'areas', 'info'),
           outputs=('counts = torch.empty', 'areas = torch.empty', 'words = torch.empty'), launches=lambda p: p['F'] > 0,
           constants='kThreads 256 faces per workgroup; info is "zeroed here"')

    BR.Row('mesh_sample_points', ('atvs_mesh_sample_scratch_size', 'atvs_mesh_sample_offsets', 'atvs_mesh_sample_place'), SAMPLE_SIZES,
           BR._mesh, BR._mesh_shapes, run=_sample_points_run, select=list, names=('points', 'colors', 'normals', 'face'),
           outputs=('points = torch.empty', 'face = torch.empty', 'colors_out = ', 'normals_out = torch.empty', 'info = torch.empty'),
           scratch=('scratch = torch.empty', 'offsets = torch.empty'), launches=lambda p: p['F'] > 1,
           constants='kThreads 256 samples per workgroup; the scan tile of 2048 faces; kStage 1024 offsets of a workgroup\'s faces in LDS')


def cases():
    """[(row name, size name)] of the two rows, for pytest's parametrize."""
    return [(name, size) for name in NAMES for size in BR.ROWS[name].sizes]
