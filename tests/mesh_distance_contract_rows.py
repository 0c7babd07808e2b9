"""The rows of ops/mesh_distance.py for the buffer contract, registered in tests/buffer_contract_rows.py's table on import: that table
must name every entry point of include/atvsnet_hip.h that writes through a pointer or takes scratch
(tests/test_buffer_contract_host.py), and these are the rows for atvs_mesh_grid_scratch_size, atvs_mesh_grid_build,
atvs_mesh_nearest_scratch_size and atvs_mesh_nearest.  tests/test_mesh_distance_host.py (the builders, without a GPU) and
tests/test_gpu_mesh_distance_contract.py (the three guarded runs) import this module and run the rows; pytest imports every test
module before it runs a test, so the table is whole whenever the suite is collected."""
import collections

import buffer_contract_rows as BR

QUERIES = 300
NAMES = ('mesh_grid', 'mesh_nearest')
# BR._mesh: vertices in [-1, 1]^3 with a NaN and an inf row, faces inside blocks of 16 vertices: a face spans up to 7 cells per axis
# at BR.RADIUS; the last size asks for the least budget (8 references per face), which forces the coarsening
GRID_SIZES = BR.merged(collections.OrderedDict((k, dict(v, m=QUERIES, max_refs=None)) for k, v in BR.MESH_SIZES.items()),
                       {'V=F=257,max_refs=8F': {'V': 257, 'F': 257, 'm': QUERIES, 'max_refs': 8 * 257}})
NEAREST_SIZES = BR.merged(GRID_SIZES, collections.OrderedDict(
    ('V=F=257,m=%d' % m, {'V': 257, 'F': 257, 'm': m, 'max_refs': None}) for m in (0, 1) + BR.AROUND_WORKGROUP))


def _inputs(p):
    return dict(BR._mesh(p, seed=41), queries=BR.cloud(p['m'], 43), max_refs=p['max_refs'])


def _shapes(p):
    return dict(BR._mesh_shapes(p), queries=((p['m'], 3), BR.F32))


def _grid_run(ops, d, place):
    grid = ops.mesh_grid(d['vertices'], d['faces'], BR.RADIUS, d['max_refs'])
    return (grid,) + ops.mesh_nearest(grid, d['queries'], closest=True)


def _nearest_run(ops, d, place):
    grid = ops.mesh_grid(d['vertices'], d['faces'], BR.RADIUS, d['max_refs'])
    grid.buf = place(grid.buf)
    return ops.mesh_nearest(grid, d['queries'], closest=True)


if NAMES[0] not in BR.ROWS:                      # (imported under two names -- as a module and by a test -- it registers once)
    BR.Row('mesh_grid', ('atvs_mesh_grid_scratch_size', 'atvs_mesh_grid_build'), GRID_SIZES, _inputs, _shapes, run=_grid_run,
           select=lambda r: list(r[1:]), names=('nearest d2', 'nearest face', 'nearest closest'),
           outputs=('info = torch.empty',), scratch=('buf = torch.empty',),          # the grid IS its scratch, as a CloudGrid's
           excluded=('MeshGrid.buf is opaque (the grid with its references in the order of arrival, a workspace of the search): compared '
                     'through mesh_nearest',),
           constants='kThreads 256 faces per workgroup; kMinCells 4096 = 8 x 512 faces; the scan tile of 2048 counters; 8 references per '
                     'face: a second and third build with a coarser cell')

    BR.Row('mesh_nearest', ('atvs_mesh_nearest_scratch_size', 'atvs_mesh_nearest'), NEAREST_SIZES, _inputs, _shapes, run=_nearest_run,
           select=list, names=('d2', 'face', 'closest'), outputs=('d2 = torch.empty', 'face = torch.empty', 'points = torch.empty'),
           scratch=('scratch = torch.empty',), launches=lambda p: p['m'] > 0,
           constants='kThreads 256 queries per workgroup; the queries\' counting sort over the grid\'s cells (scan tile 2048)')


def cases():
    """[(row name, size name)] of the two rows, for pytest's parametrize."""
    return [(name, size) for name in NAMES for size in BR.ROWS[name].sizes]
