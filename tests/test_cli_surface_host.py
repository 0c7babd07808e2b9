"""The command-line surface of the ETH3D driver and of the tools it shares option groups with, on the host (no GPU), against
tests/golden/cli_surface.json, which was recorded from the code before the groups had one owner each: every parser's actions
(option strings, dest, nargs, const, default, type, choices, required, metavar -- help text is left out: shared definitions may
merge their wording), every refused command line with its exit code and the message after `error: `, the driver's _run_options
for a command line that turns every group on, and _option_rules' rows, in order, with every conditional row present."""
import json
import os

import pytest

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS
from atvsnet_amd.atvsnet import depth_fusion, eval_cloud, eval_depth, eval_pointcloud, mesh_fusion

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, 'golden', 'cli_surface.json')) as _f:
    GOLDEN = json.load(_f)
TOOLS = dict(eval_pointcloud=eval_pointcloud, mesh_fusion=mesh_fusion, eval_depth=eval_depth, depth_fusion=depth_fusion,
             eval_cloud=eval_cloud)


@pytest.fixture
def flags():
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


def _surface(parser):
    rows = [[list(a.option_strings), a.dest, a.nargs, a.const, a.default, None if a.type is None else a.type.__name__,
             None if a.choices is None else list(a.choices), a.required, list(a.metavar) if isinstance(a.metavar, tuple) else a.metavar]
            for a in parser._actions]
    return json.loads(json.dumps(sorted(rows, key=lambda r: r[0])))


@pytest.mark.parametrize('tool', sorted(TOOLS))
def test_the_parsers_declare_what_they_declared(flags, tool):
    got, want = _surface(TOOLS[tool].make_parser()), GOLDEN['surface'][tool]
    assert [r[0] for r in got] == [r[0] for r in want]
    for g, w in zip(got, want):
        assert g == w


@pytest.mark.parametrize('tool', sorted(GOLDEN['refused']))
def test_refused_command_lines_keep_their_message(flags, capsys, tool):
    assert len(GOLDEN['refused'][tool]) >= (60 if tool == 'eval_pointcloud' else 12)
    for case in GOLDEN['refused'][tool]:
        with pytest.raises(SystemExit) as e:
            TOOLS[tool].cli([os.path.join(HERE, 'golden') if a == '{dir}' else a for a in case['argv']])
        err = ' '.join(capsys.readouterr().err.split())
        assert e.value.code == case['code'] == 2, case['argv']
        assert err[err.index('error: ') + len('error: '):] == case['message'], case['argv']


def test_every_group_at_once_gives_the_same_run_options(flags):
    case = GOLDEN['run_options']
    got = eval_pointcloud._run_options(eval_pointcloud.make_parser().parse_args(case['argv']))
    assert json.loads(json.dumps(got)) == case['options']
    assert got['mesh']['carve_weight'] == mesh_fusion.DEFAULT_CARVE_WEIGHT


def test_option_rules_keep_their_rows_order_and_bytes():
    assert len(GOLDEN['option_rules'][0]['rules']) == 6 + 11 and len(GOLDEN['option_rules'][-1]['rules']) == 6
    for case in GOLDEN['option_rules']:
        rules = eval_pointcloud._option_rules(**case['options'])
        assert [[bool(b), m] for b, m in rules] == case['rules']
