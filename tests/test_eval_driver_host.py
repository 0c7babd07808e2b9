"""The ETH3D driver's scene loop and option rules on the host (no GPU): eth3d_maps._run_scene over a fake map source -- the
order of load / submit / finish, the files, writer errors, TIMES -- and _option_rules through run_eval_pc and cli."""
import itertools
import os

import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd import FLAGS
from atvsnet_amd.atvsnet import eth3d_maps, eval_pointcloud as E

MAPS = 3
MAP_FILES = ['%08d%s' % (10 * (i + 1), ext) for i in range(MAPS) for ext in ('.pfm', '_prob.pfm', '.jpg', '.txt', '.png')]
DEFAULT_KEYS = {'prepare', 'submit', 'wait', 'write', 'maps'}


@pytest.fixture
def flags():
    FLAGS.reset()
    yield FLAGS
    FLAGS.reset()


class FakeSource(object):
    """Three maps, two slots; map i has out_index 10 * (i + 1), fixed 8x10 outputs and a 32x40 image.  Records every call."""
    SLOTS = 2

    def __init__(self, extra_times=None):
        self.log, self.queued, self.extra_times = [], [], extra_times or {}

    def begin_scene(self, mvs_list):
        self.log.append('begin %d' % len(mvs_list))

    def end_scene(self):
        self.log.append('end')
        return dict(self.extra_times)

    def room(self):
        return len(self.queued) < self.SLOTS

    def load(self, i):
        self.log.append('load %d' % i)
        return i

    def submit(self, loaded):
        self.log.append('submit %d' % loaded)
        self.queued.append(loaded)

    def finish(self, stage):
        i = self.queued.pop(0)
        self.log.append('finish %d' % i)
        rng = np.random.default_rng(i)
        outputs = [rng.uniform(-0.1 if k < 2 else 0.0, 1.0, (1, 8, 10, 1)).astype(np.float32) for k in range(4)]     # some depths <= 0
        image = rng.integers(0, 256, (32, 40, 3), dtype=np.uint8)
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3], cam[1, 3] = np.eye(4), [[50 + i, 0, 5], [0, 50, 4], [0, 0, 1]], (0.1, 0.01, 16, 0.9)
        if stage is not None:
            stage(10 * (i + 1), outputs[0], outputs[2], image, cam)
        return 10 * (i + 1), outputs, image, cam

    def close(self):
        self.log.append('close')


def _tree(folder):
    return {os.path.relpath(os.path.join(d, f), folder): open(os.path.join(d, f), 'rb').read()
            for d, _, files in os.walk(folder) for f in files}


def test_call_order_files_and_times(flags, tmp_path):
    """The next map is loaded and submitted before the oldest is finished; five files per map and zz_runtime.txt, the same bytes
    from the writer thread as from the caller; TIMES has the documented keys, the source's and a timed writer's on top."""
    trees = {}
    for threaded in (False, True):
        source = FakeSource()
        out = str(tmp_path / ('threaded' if threaded else 'inline'))
        fusion, map_cams, seconds = E._run_scene(source, [None] * MAPS, out, E._Writer(threaded))
        assert fusion is None and map_cams == {} and seconds > 0
        assert [c for c in source.log if not c.startswith('load')] == [
            'begin 3', 'submit 0', 'submit 1', 'finish 0', 'submit 2', 'finish 1', 'finish 2', 'end']
        assert [c for c in source.log if not c.startswith('submit')][1:6] == ['load 0', 'load 1', 'load 2', 'finish 0', 'finish 1']
        assert set(E.TIMES) == DEFAULT_KEYS and E.TIMES['maps'] == MAPS
        trees[threaded] = _tree(out)
        assert sorted(trees[threaded]) == sorted(['zz_runtime.txt'] + [os.path.join('depths_atvsnet', f) for f in MAP_FILES])
        assert trees[threaded].pop('zz_runtime.txt').startswith(b'runtime ')
    assert trees[False] == trees[True]

    source = FakeSource(extra_times={'upload': 0.5, 'gpu_ms': [1.0, 2.0, 3.0]})
    E._run_scene(source, [None] * MAPS, str(tmp_path / 'nofiles'), E._Writer(True, timed=True), map_files=False)
    assert sorted(_tree(str(tmp_path / 'nofiles'))) == ['zz_runtime.txt']
    assert set(E.TIMES) == DEFAULT_KEYS | {'writer_busy', 'upload', 'gpu_ms'} and E.TIMES['maps'] == MAPS
    assert E.TIMES['writer_busy'] == 0.0 and E.TIMES['upload'] == 0.5 and E.TIMES['gpu_ms'] == [1.0, 2.0, 3.0]


def test_stage_runs_once_per_map_before_its_files(flags, tmp_path, monkeypatch):
    out, bare = str(tmp_path / 'out'), str(tmp_path / 'bare')
    made, folder = [], [out]

    class FakeFusion(object):
        def __init__(self, n_maps, rows, cols, device, **fuse):
            self.args, self.added = (n_maps, rows, cols, device, fuse), []
            made.append(self)

        def add(self, out_index, depth, prob, image, cam, stream=None):
            assert not [f for f in _tree(folder[0]) if os.path.basename(f).startswith('%08d' % out_index)]
            assert depth.min() <= 0 and np.isfinite(depth).all()          # not yet rewritten by the inverse-depth step
            self.added.append((out_index, stream))

    monkeypatch.setattr(E.depth_fusion, 'SceneFusion', FakeFusion)
    fusion, map_cams, _ = E._run_scene(FakeSource(), [None] * MAPS, out, E._Writer(False), fuse=dict(prob_threshold=0.5),
                                       keep_cams=True, device='dev')
    assert made == [fusion] and fusion.args == (MAPS, 32, 40, 'dev', dict(prob_threshold=0.5))
    assert fusion.added == [(10, None), (20, None), (30, None)]
    assert sorted(map_cams) == [10, 20, 30] and all(c.dtype == np.float64 and c.shape == (2, 4, 4) for c in map_cams.values())
    assert map_cams[20][1, 0, 0] == 51.0
    assert len(_tree(out)) == 1 + len(MAP_FILES)
    made[:], folder[0] = [], bare
    fusion, map_cams, _ = E._run_scene(FakeSource(), [None] * MAPS, bare, E._Writer(False), fuse=dict(), map_files=False)
    assert made == [fusion] and len(fusion.added) == MAPS and map_cams == {} and sorted(_tree(bare)) == ['zz_runtime.txt']


@pytest.mark.parametrize('scene_cache, write_thread', [(False, True), (True, True), (True, False)])
def test_a_write_error_surfaces_and_the_source_is_closed(flags, tmp_path, monkeypatch, scene_cache, write_thread):
    """run_eval_pc over the fake source: an exception inside the second map's write job comes out of run_eval_pc, from the writer
    thread too, and the source is closed."""
    dense = tmp_path / 'scene'
    dense.mkdir()
    (dense / 'pair.txt').write_text('3\n' + ''.join('%d\n2 %d 1.0 %d 1.0\n' % (i, (i + 1) % 3, (i + 2) % 3) for i in range(3)))
    source = FakeSource()
    written = []

    def write_map(output_folder, out_index, *rest):
        if out_index == 20:
            raise OSError('disk full at %d' % out_index)
        written.append(out_index)

    monkeypatch.setattr(eth3d_maps, '_write_map', write_map)
    monkeypatch.setattr(E.example, '_load_weights', lambda: None)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda device: None)
    monkeypatch.setattr(E, '_SceneSource' if scene_cache else '_PipelineSource', lambda *args: source)
    with pytest.raises(OSError, match='disk full at 20'):
        E.run_eval_pc(str(tmp_path / 'out'), [[[str(dense), str(dense / 'images'), 'toy'], 'preprocessed']], scene_cache=scene_cache,
                      write_thread=write_thread)
    assert source.log[-1] == 'close' and source.log.count('close') == 1 and written == [10]
    assert not os.path.exists(str(tmp_path / 'out' / 'toy' / 'zz_runtime.txt'))


ON = dict(use_graph=False, scene_cache=True, fuse=dict(prob_threshold=0.8, disp_threshold=0.01, num_consistent=2), map_files=False,
          gt_ply=['g.ply'], register=dict(with_scale=False, init_cameras=None), clean=dict(voxel=0.1),
          score_maps=dict(splat=E.eval_depth.DEFAULT_SPLAT, occlusion_tol=E.eval_depth.DEFAULT_OCCLUSION_TOL,
                          pixel_centre=E.eval_depth.DEFAULT_PIXEL_CENTRE))
OFF = dict(use_graph=True, scene_cache=False, fuse=None, map_files=True, gt_ply=None, register=None, clean=None, score_maps=None)
ARGV = dict(use_graph=['--eager'], scene_cache=['--scene_cache'], fuse=['--fuse'], map_files=['--no_map_files'], gt_ply=['--gt_ply', 'g.ply'],
            register=['--register'], clean=['--clean_voxel', '0.1'], score_maps=['--score_maps'])


def test_every_option_rule_is_refused_alike_by_run_eval_pc_and_cli(flags, capsys):
    """Every rule of _option_rules, found by calling it over all on/off settings of the options: the first setting that breaks
    that rule before any other is refused by run_eval_pc (ValueError) and by cli (exit 2) with the same message."""
    assert not any(broken for broken, _ in E._option_rules()) and not any(broken for broken, _ in E._option_rules(**OFF))
    first = {}
    for chosen in itertools.product((False, True), repeat=len(ON)):
        options = {k: (ON if on else OFF)[k] for k, on in zip(sorted(ON), chosen)}
        rules = E._option_rules(**options)
        broken = [k for k, (b, _) in enumerate(rules) if b]
        if broken:
            first.setdefault(broken[0], (options, rules[broken[0]][1]))
    assert sorted(first) == list(range(len(E._option_rules()))) and len(first) >= 6
    assert len({message for _, message in first.values()}) == len(first)
    for options, message in first.values():
        with pytest.raises(ValueError) as e:
            E.run_eval_pc('out', [], **options)
        assert str(e.value) == message
        argv = [a for k in sorted(options) if options[k] is not OFF[k] for a in ARGV[k]]
        with pytest.raises(SystemExit) as e:
            E.cli(argv)
        assert e.value.code == 2 and message in ' '.join(capsys.readouterr().err.split()), argv
    assert not os.path.exists('out')
