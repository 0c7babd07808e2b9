"""tests/buffer_contract_rows.py is complete and its builders do what they state, without a GPU: every entry point that
include/atvsnet_hip.h declares from atvs_fusibile onwards and that writes through a pointer or takes scratch is named by a row (the
seven network-side kernels declared behind that line by a row of tests/network_contract_rows.py: there is no exclusion list), every *_scratch_size query sits in a row beside its partner, every row names a
size that reaches each of its entry points, and every builder returns inputs of the stated shapes and dtypes, the same ones twice."""
import inspect
import re

import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import _lib

import buffer_contract_rows as BR
import network_contract_rows as NR

FIRST = 'atvs_fusibile'
QUERIES = ('_size', '_supported', '_grid')


def _declarations():
    """[(name, [parameter text])] of include/atvsnet_hip.h in its order; the names are those `_lib.prototypes()` reads."""
    with open(_lib.HEADER) as f:
        text = re.sub(r'/\*.*?\*/|//[^\n]*|^[ \t]*#.*?$', '', f.read(), flags=re.S | re.M)
    found = [(m.group(1), [' '.join(a.split()) for a in m.group(2).split(',')])
             for m in re.finditer(r'\b(atvs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)]
    assert sorted(n for n, _ in found) == sorted(_lib.prototypes())
    return found


def _in_scope():
    decl = _declarations()
    names = [n for n, _ in decl]
    return decl[names.index(FIRST):]


def _writes(params):
    return any('*' in a and not a.startswith('const ') for a in params) or any(re.search(r'\bscratch$', a) for a in params)


def _named():
    named = set()
    for row in BR.ROWS.values():
        named.update(row.entries)
        for p in row.sizes.values():
            named.update(p.get('entries', ()))
    return named


def test_the_scope_begins_where_the_issue_says_and_is_not_empty():
    scope = [n for n, _ in _in_scope()]
    assert scope[0] == FIRST and len(scope) > 80
    assert 'atvs_mesh_cluster_faces' in scope and 'atvs_cloud_grid_build' in scope
    assert any('atvs_conv3d_b_f32' in row.entries for row in NR.ROWS.values())          # is in the network table


def test_every_entry_point_that_writes_is_in_a_row_and_nothing_is_excluded():
    named = _named()
    network = set(e for row in NR.ROWS.values() for e in row.entries)
    writers = [n for n, params in _in_scope() if _writes(params) and not n.endswith(QUERIES)]
    assert len(writers) > 50
    behind = [n for n in writers if n not in named]            # the network-side kernels declared behind atvs_fusibile, and their packers
    assert all(re.match(r'atvs_(deconv_up|conv_c16b?)_', n) for n in behind), 'no row of tests/buffer_contract_rows.py names %s' % behind
    uncovered = [n for n in behind if n not in network and not n.endswith('_pack')]
    assert not uncovered, 'no row of tests/network_contract_rows.py names %s' % uncovered
    # there are no exclusions
    assert BR.EXCLUDED_ENTRY_POINTS == {}


def test_every_name_a_row_uses_is_declared():
    declared = set(_lib.prototypes())
    assert _named() <= declared, sorted(_named() - declared)


def test_every_scratch_size_query_has_its_partner_in_a_row():
    queries = [n for n, _ in _in_scope() if n.endswith('_scratch_size')]
    assert len(queries) >= 20
    for q in queries:
        stem = q[:-len('_scratch_size')]
        rows = [row for row in BR.ROWS.values() if q in row.entries]
        assert rows, 'no row reaches %s' % q
        # (atvs_cloud_radius_count takes atvs_cloud_knn's scratch, "the same scratch": one row with the partner is enough)
        partners = [e for row in rows for e in row.entries if e.startswith(stem) and not e.endswith('_scratch_size')]
        assert partners, '%s is in no row beside the entry point it sizes the scratch of' % q
        for row in rows:
            assert row.scratch, '%s names %s but lists no scratch allocation' % (row.name, q)


def test_every_row_names_a_size_that_reaches_each_entry_point():
    for row in BR.ROWS.values():
        somewhere = set()
        for size in row.sizes:
            somewhere.update(row.required(size))
        assert set(row.entries) <= somewhere, (row.name, sorted(set(row.entries) - somewhere))


def test_every_ops_function_of_the_scope_has_a_row():
    from atvsnet_amd.ops import aanet, cloud, colmap, mesh, mesh_simplify, mesh_topology, prepare, tsdf
    wanted = []
    for module in (cloud, mesh, mesh_topology, mesh_simplify, tsdf, colmap):
        wanted += [n for n, f in vars(module).items() if inspect.isfunction(f) and f.__module__ == module.__name__ and not n.startswith('_')]
    wanted += ['prepare_view', 'fusibile', 'fusion_stage', 'depth_normals', 'fusibile_scene', 'fusion_support']
    assert all(hasattr(prepare, n) or hasattr(aanet, n) for n in wanted[-6:])
    assert len(wanted) >= 43
    missing = [n for n in wanted if n not in BR.ROWS]
    assert not missing, missing


def test_every_exclusion_of_a_selection_quotes_a_header_line_that_says_so():
    with open(_lib.HEADER) as f:
        lines = f.read().split('\n')
    for row in BR.ROWS.values():
        for text in row.excluded:
            m = re.search(r'"([^"]+)".*?header line (\d+)', text, flags=re.S)
            if m is None:
                assert 'intermediates' in text or 'workspace' in text, (row.name, text)         # not an output of the C call at all
                continue
            quote, line = ' '.join(m.group(1).replace('...', '\0').split()), int(m.group(2))
            near = ' '.join(' '.join(l.strip().lstrip('*').strip() for l in lines[line - 2:line + 2]).split())
            for part in quote.split('\0'):
                assert part.strip().strip(',') in near, '%s: header line %d does not say %r' % (row.name, line, part)


@pytest.mark.parametrize('name,size', BR.cases(), ids=['%s[%s]' % c for c in BR.cases()])
def test_builder(name, size):
    row = BR.ROWS[name]
    p = row.sizes[size]
    d, again = row.build(p), row.build(p)
    stated = row.shapes(p)
    tensors = {k: v for k, v in d.items() if isinstance(v, torch.Tensor)}
    assert sorted(tensors) == sorted(stated), (sorted(tensors), sorted(stated))
    for k, (shape, dtype) in stated.items():
        t = tensors[k]
        assert t.device.type == 'cpu' and t.dtype == dtype and t.is_contiguous(), (k, t.dtype, t.device)
        if shape is not None:
            assert tuple(t.shape) == tuple(shape), (k, tuple(t.shape), shape)
        assert t.dim() == 0 or int(t.shape[0]) <= 5000                     # nothing above about 5,000 points, faces or blocks
        a, b = t.contiguous().view(torch.uint8) if t.numel() else t, again[k].contiguous().view(torch.uint8) if t.numel() else again[k]
        assert torch.equal(a, b), '%s is not deterministic' % k
    for k, v in d.items():
        if not isinstance(v, torch.Tensor):
            assert again[k] == v or v is None
    assert set(row.writable) <= set(tensors)
    assert row.names and row.constants
