"""The rows of ops/mesh_smooth.py for the buffer contract, registered in tests/buffer_contract_rows.py's table on import: that
table must name every entry point of include/atvsnet_hip.h that writes through a pointer or takes scratch
(tests/test_buffer_contract_host.py), and these are the rows for atvs_mesh_adjacency_scratch_size, atvs_mesh_adjacency,
atvs_mesh_quantize, atvs_mesh_smooth_pass, atvs_mesh_dequantize, atvs_mesh_face_extent, atvs_mesh_vertex_normal_sums and
atvs_mesh_vertex_normals, and two for the composites ops.mesh_smooth and ops.mesh_vertex_normals.  tests/test_mesh_smooth_host.py
(the builders, without a GPU) and tests/test_gpu_mesh_smooth_contract.py (the three guarded runs) import this module and run the
rows; pytest imports every test module before it runs a test, so the table is whole whenever the suite is collected."""
import collections

import numpy as np

import buffer_contract_rows as BR
import mesh_smooth_restated as R

ORIGIN, STEP = (0.0, 0.0, 0.0), 2.0 ** -30         # BR._mesh's vertices lie in [-1, 1]: |q| <= 2^30
FACTORS = (0.5, -0.53)
NAMES = ('mesh_adjacency', 'mesh_quantize', 'mesh_smooth_pass', 'mesh_dequantize', 'mesh_face_extent', 'mesh_vertex_normal_sums',
         'mesh_normals_from_sums', 'mesh_smooth', 'mesh_vertex_normals')
ADJACENCY_SIZES = BR.merged(BR.MESH_SIZES, collections.OrderedDict(('V=F=%d' % v, {'V': v, 'F': v}) for v in (BR.CENSUS_MIN_FACES, BR.CENSUS_MIN_FACES + 1)))
_SMOOTH = ('atvs_mesh_adjacency_scratch_size', 'atvs_mesh_adjacency', 'atvs_mesh_quantize', 'atvs_mesh_smooth_pass', 'atvs_mesh_dequantize')
_NORMALS = ('atvs_mesh_face_extent', 'atvs_mesh_vertex_normal_sums', 'atvs_mesh_vertex_normals')


def _words(info):
    return BR._t([info[k] for k in R.ADJACENCY_INFO], np.int64)


def _adjacency_select(r):
    offsets = r.offsets.cpu().numpy()
    return [r.degree, r.flags, r.offsets, BR._t(R.sorted_rows(offsets, r.neighbours.cpu().numpy())), _words(r.info)]


def _placed_adjacency(ops, d, place):
    a = ops.mesh_adjacency(d['vertices'], d['faces'])
    return ops.MeshAdjacency(place(a.degree), place(a.flags), place(a.offsets), place(a.neighbours), a.info)


def _passes(ops, d, place):
    adjacency = _placed_adjacency(ops, d, place)
    q0 = place(ops.mesh_quantize(d['vertices'], ORIGIN, STEP)[0])
    q1, tallies = ops.mesh_smooth_pass(q0, adjacency, FACTORS[0], ops.MESH_FLAG_BOUNDARY)
    q2, tallies = ops.mesh_smooth_pass(place(q1), adjacency, FACTORS[1], 0, tallies)
    return q0, q1, q2, tallies


def _dequantize_run(ops, d, place):
    q0, _, q2, _ = _passes(ops, d, place)
    return ops.mesh_dequantize(place(q2), q0, d['vertices'], ORIGIN, STEP)


def _extent_select(r):
    return [BR._t([r['max_extent']], np.float64), BR._t([r[k] for k in ('usable_faces', 'skipped_index_faces', 'nonfinite_faces')], np.int64)]


def _smooth_select(r):
    out, info = r
    return [out, _words(info), BR._t(info['origin'] + [info['step']], np.float64), BR._t([info['passes'], info['nonfinite_vertices']], np.int64)]


if NAMES[0] not in BR.ROWS:                      # (imported under two names -- as a module and by a test -- it registers once)
    BR.Row('mesh_adjacency', ('atvs_mesh_adjacency_scratch_size', 'atvs_mesh_adjacency'), ADJACENCY_SIZES, BR._mesh, BR._mesh_shapes,
           run=lambda ops, d, place: ops.mesh_adjacency(d['vertices'], d['faces']), select=_adjacency_select,
           names=('degree', 'flags', 'offsets', 'neighbours[:offsets[V]], every row sorted', 'info'),
           outputs=('degree = torch.empty', 'flags = torch.empty', 'offsets = torch.empty', 'neighbours = torch.empty', 'words = torch.empty'),
           scratch=('scratch = torch.empty',), launches=lambda p: p['V'] > 0,
           excluded=('entries offsets[V].. of neighbours: "the first offsets[n_vertices] entries are written", header line 1617',
                     'the order inside a row of neighbours: "in an ORDER THAT IS NOT DEFINED", header line 1618: the rows are compared sorted'),
           constants='kThreads 256 faces / vertices / slots per workgroup; the table of max(6 n_faces, ATVS_MESH_ADJACENCY_MIN_SLOTS 1024) '
                     'slots: 170 | 171 faces; the scan tile of 2048 vertices')

    BR.Row('mesh_quantize', ('atvs_mesh_quantize',), BR.MESH_SIZES, BR._mesh, BR._mesh_shapes,
           run=lambda ops, d, place: ops.mesh_quantize(d['vertices'], ORIGIN, STEP),
           select=lambda r: [r[0], BR._t([r[1]['nonfinite_vertices']], np.int64)], names=('q', 'nonfinite_vertices'),
           outputs=('q = torch.empty', 'words = torch.empty'), launches=lambda p: p['V'] > 0, constants='kThreads 256 vertices per workgroup')

    BR.Row('mesh_smooth_pass', ('atvs_mesh_smooth_pass',), BR.MESH_SIZES, BR._mesh, BR._mesh_shapes, run=_passes, select=lambda r: list(r[1:]),
           names=('q after a pinned lam pass', 'q after a mu pass', 'the running tallies'), outputs=('q_out = torch.empty_like', 'info = torch.zeros'),
           launches=lambda p: p['V'] > 0, constants='kThreads 256 vertices per workgroup; info is the caller\'s, zeroed once and added to')

    BR.Row('mesh_dequantize', ('atvs_mesh_dequantize',), BR.MESH_SIZES, BR._mesh, BR._mesh_shapes, run=_dequantize_run, select=lambda r: [r],
           names=('vertices_out',), outputs=('vertices_out = torch.empty_like',), launches=lambda p: p['V'] > 0,
           constants='kThreads 256 coordinates per workgroup: 3 V is no multiple of 256')

    BR.Row('mesh_face_extent', ('atvs_mesh_face_extent',), BR.MESH_SIZES, BR._mesh, BR._mesh_shapes,
           run=lambda ops, d, place: ops.mesh_face_extent(d['vertices'], d['faces']), select=_extent_select, names=('max_extent', 'counts'),
           outputs=('words = torch.empty',), launches=lambda p: p['F'] > 0, constants='kThreads 256 faces per workgroup; info is "zeroed here"')

    BR.Row('mesh_vertex_normal_sums', ('atvs_mesh_vertex_normal_sums',), BR.MESH_SIZES, BR._mesh, BR._mesh_shapes,
           run=lambda ops, d, place: ops.mesh_vertex_normal_sums(d['vertices'], d['faces'], 0.5), select=list, names=('sums', 'incidences'),
           outputs=('sums = torch.empty', 'incidences = torch.empty', 'info = torch.empty'), launches=lambda p: p['V'] > 0 or p['F'] > 0,
           constants='kThreads 256 faces per workgroup; both outputs are "zeroed here"; faces larger and smaller than the area unit 0.5')

    BR.Row('mesh_normals_from_sums', ('atvs_mesh_vertex_normals',), BR.MESH_SIZES, BR._mesh, BR._mesh_shapes,
           run=lambda ops, d, place: ops.mesh_normals_from_sums(place(ops.mesh_vertex_normal_sums(d['vertices'], d['faces'], 0.5)[0])),
           select=lambda r: [r], names=('normals',), outputs=('normals = torch.empty',), launches=lambda p: p['V'] > 0,
           constants='kThreads 256 vertices per workgroup')

    BR.Row('mesh_smooth', _SMOOTH, BR.MESH_SIZES, BR._mesh, BR._mesh_shapes,
           run=lambda ops, d, place: ops.mesh_smooth(d['vertices'], d['faces'], 2, FACTORS[0], FACTORS[1]), select=_smooth_select,
           names=('vertices_out', 'the adjacency\'s words', 'origin and step', 'passes, nonfinite_vertices'),
           outputs=('degree = torch.empty', 'neighbours = torch.empty', 'q = torch.empty', 'tallies = torch.zeros', 'q_out = torch.empty_like',
                    'vertices_out = torch.empty_like'),
           scratch=('scratch = torch.empty',), launches=lambda p: p['V'] > 0,
           constants='as the rows of its four steps; two iterations ping-pong four q buffers')

    BR.Row('mesh_vertex_normals', _NORMALS, BR.MESH_SIZES, BR._mesh, BR._mesh_shapes,
           run=lambda ops, d, place: ops.mesh_vertex_normals(d['vertices'], d['faces']), select=lambda r: [r], names=('normals',),
           outputs=('words = torch.empty', 'sums = torch.empty', 'normals = torch.empty'), launches=lambda p: p['F'] > 0,
           constants='as the rows of its three steps; the area unit is the device\'s largest s')


def cases():
    """[(row name, size name)] of the rows, for pytest's parametrize."""
    return [(name, size) for name in NAMES for size in BR.ROWS[name].sizes]
