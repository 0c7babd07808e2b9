"""The range guard on the host (no GPU): the suspect rule of the maps in flight on stand-in queues and a fake flag, the guard's
messages, and the names atvsnet/example.py re-exports from the inference runtime's modules."""
import numpy as np
import pytest
import torch

import atvsnet_amd  # noqa: F401
from atvsnet_amd.atvsnet import example, graphs, pipeline, range_guard

RANGE_HINT = ('an activation or weight left the fp16 range of the split-operand kernels (or the inputs were not finite); rerun with '
              'ATVS_SPLIT16=0 for the fp32 kernels')


class Queue(object):
    def __init__(self, busy):
        self.busy, self.suspect = list(busy), set()


class Flag(object):
    """The sticky flag: a read returns it and clears it."""

    def __init__(self, up):
        self.up, self.reads = up, []

    def __call__(self, device):
        self.reads.append(device)
        up, self.up = self.up, False
        return up


@pytest.fixture
def syncs(monkeypatch):
    calls = []
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda device=None: calls.append(device))
    return calls


def test_flag_down_marks_nothing(syncs):
    a, b, flag = Queue([True, False]), Queue([False, True]), Flag(False)
    assert range_guard.mark_suspects('dev', [a, b], read_flag=flag) is False
    assert a.suspect == set() and b.suspect == set()
    assert flag.reads == ['dev'] and syncs == []


def test_flag_up_marks_every_busy_slot_of_every_queue_once(syncs):
    a, b, flag = Queue([True, False]), Queue([False, True]), Flag(True)
    assert range_guard.mark_suspects('dev', [a, b], read_flag=flag) is True
    assert a.suspect == {0} and b.suspect == {1}
    assert flag.reads == ['dev', 'dev'] and syncs == ['dev']        # the second read, after the synchronize, is the clear
    assert not flag.up
    # after the clear: nothing more is marked, whatever is busy by now
    a.busy[1] = True
    assert range_guard.mark_suspects('dev', [a, b], read_flag=flag) is False
    assert a.suspect == {0} and b.suspect == {1}
    assert len(flag.reads) == 3 and syncs == ['dev']


def test_guard_messages_are_the_recorded_ones(monkeypatch):
    with pytest.raises(FloatingPointError) as e:
        range_guard.check_finite(np.array([1.0, np.nan, np.inf]), flag=False)
    assert str(e.value) == 'depth map holds 2 non-finite values: ' + RANGE_HINT
    monkeypatch.setattr(range_guard.ops, 'nonfinite_seen', lambda device: True)
    with pytest.raises(FloatingPointError) as d:
        range_guard.check_device('dev')
    assert str(d.value) == 'a batch norm saw non-finite moments: ' + RANGE_HINT
    assert 'ATVS_SPLIT16=0' in str(e.value) and 'ATVS_SPLIT16=0' in str(d.value)
    assert range_guard.check_finite(np.ones(3), flag=False).shape == (3,)


REEXPORTS = {pipeline: ['depth_range', 'infer_twoview', 'multiview_towers', 'infer_multiview_from_features', 'infer_multiview'],
             graphs: ['GraphedInference', 'cu_split_streams', 'PipelinedInference'],
             range_guard: ['check_device', 'check_finite', 'infer_checked', '_fallback_logged']}


@pytest.mark.parametrize('home, name', [(m, n) for m, names in REEXPORTS.items() for n in names])
def test_example_reexports_the_runtime(home, name):
    assert getattr(example, name) is getattr(home, name)


def test_the_fallback_log_is_one_list():
    assert example._fallback_logged is range_guard._fallback_logged
    assert example._load_weights.__module__ == example.__name__          # the drivers' tests patch it there
