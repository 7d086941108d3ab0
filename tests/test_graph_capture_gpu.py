"""The inference paths' graph capture (matcha/_graphs.py) with a process group up, as when a data-parallel training
process renders a sample between epochs: the capture takes the thread_local mode the train step takes, and the
replays are bitwise the eager runs."""
from __future__ import annotations

import os
import socket

import pytest
import torch
import torch.distributed as dist

import griffinlim_ref as R
from golden.weights_recipe import apply_recipe
from hifi_gan import AttrDict, Generator
from hifigan_ref import CONFIGS
from matcha._graphs import capture_mode
from matcha.utils.audio_process import GriffinLim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture
def world1():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    yield
    dist.destroy_process_group()


def test_vocoder_graph_under_a_process_group(world1):
    assert capture_mode() == "thread_local"
    m = Generator(AttrDict(CONFIGS["v3_small"]))
    apply_recipe(m, 5)
    m = m.to(DEV).eval()
    mel = (torch.randn(1, 80, 11, generator=torch.Generator().manual_seed(4)) * 1.5 - 5.5).to(DEV)
    with torch.no_grad():
        first, again = m(mel), m(mel)  # captures and replays, then replays
        assert len(m._graphs) == 1
        m.graph = False
        want = m(mel)
    assert want.shape == (1, 1, 11 * m.hop) and want.any()
    assert torch.equal(first, want) and torch.equal(again, want)


def test_griffinlim_graph_under_a_process_group(world1):
    assert capture_mode() == "thread_local"
    kw = dict(n_fft=1024, n_iter=2, hop_length=256, win_length=1024, power=1.0)
    gl, eager = GriffinLim(**kw), GriffinLim(**kw)
    eager.graph = False
    c = R.case(1, 5)
    lin, ang = c["lin"].to(DEV), c["angles_rand"].to(DEV)
    got, want = gl(lin, angles=ang), eager(lin, angles=ang)
    assert len(gl._graphs) == 1 and not eager._graphs
    assert want.shape == (1, 4 * 256) and want.any()
    assert torch.equal(got, want)
