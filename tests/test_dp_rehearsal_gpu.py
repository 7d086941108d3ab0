"""What bench.py's N>1 leg adds on top of the captured data-parallel step of tests/test_dp_gpu.py, rehearsed on one
GPU with a world-size-1 RCCL group (RCCL refuses two ranks on one device, so one rank is the only place this code
runs before a multi-GPU node runs it): the device progress markers (csrc/dp_comm.cpp progress_mark_kernel,
matcha.watchdog.DeviceProgress) eagerly, captured on their own and captured inside the step's graph; the watchdog
reading a real device object; Trainer.measure_dp_tail; and the eager bucketed step over RCCL with the all-reduces
forked onto the reducer stream.  With one rank the exchange is an identity and every kernel on the path is
fixed-order, so every expectation is an exact integer or a bitwise comparison."""
from __future__ import annotations

import math
import os
import socket

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S = 4  # steps of the shared runs


def _model(seed=0):
    from matcha.models.matcha_tts import MatchaTTS

    torch.manual_seed(seed)
    m = MatchaTTS(n_vocab=150, out_channels=80, hidden_channels=192).to(DEV)
    m.eval()
    return m


def _inject(m, t, z):
    m.decoder.compute_loss_and_prior = (lambda f: (lambda *a, **k: f(*a, **{**k, "t": t, "z": z})))(
        m.decoder.compute_loss_and_prior)


@pytest.fixture(scope="module")
def world1():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    yield
    dist.destroy_process_group()


def _trainer(cfg, force_dp: bool = False, progress: bool = False):
    """The model, t / z injection and batch of tests/test_dp_gpu.py::_run under `cfg`."""
    from matcha.training import Trainer, synthetic_batch
    from matcha.watchdog import DeviceProgress

    b = synthetic_batch(4, 24, 96, seed=3, device=DEV)
    m = _model(11)
    t = torch.rand(4, 1, 1, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    z = torch.randn(4, 80, 96, generator=torch.Generator(device=DEV).manual_seed(2), device=DEV)
    _inject(m, t, z)
    old = Trainer.force_dp
    Trainer.force_dp = force_dp
    try:
        tr = Trainer(m, cfg)
    finally:
        Trainer.force_dp = old
    if progress:
        tr.progress = DeviceProgress()  # before the first step, as bench.py wires it
    return tr, m, b


def _params(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def _steps(tr, b, n):
    logs = [tr.step([b]).clone() for _ in range(n)]
    torch.cuda.synchronize()
    return logs


def _graph_cfg(comm):
    from matcha.training import TrainConfig

    return TrainConfig(graph=True, comm=comm, bucket_mb=4.0)


@pytest.fixture(scope="module")
def rccl_progress_run(world1):
    """S captured DP steps over RCCL with a progress object wired, a StepWatchdog polling it the whole time."""
    from matcha.watchdog import StepWatchdog

    tr, m, b = _trainer(_graph_cfg("rccl"), force_dp=True, progress=True)
    # the bound is far above anything this can take: a firing watchdog ends the process (os._exit)
    wd = StepWatchdog(rank=0, bound_s=600, device=tr.progress, poll_s=0.05)
    try:
        logs = _steps(tr, b, S)
        read = tr.progress.read()
        report = wd.report(0.0)
        fired = wd.fired
    finally:
        wd.stop()
    out = dict(tr=tr, logs=torch.stack(logs), params=_params(m), read=read, report=report, fired=fired,
               wd_alive=wd._t.is_alive())
    yield out
    tr.progress.close()


@pytest.fixture(scope="module")
def rccl_plain_run(world1):
    """The same S steps without a progress object."""
    tr, m, b = _trainer(_graph_cfg("rccl"), force_dp=True)
    logs = _steps(tr, b, S)
    return dict(tr=tr, logs=torch.stack(logs), params=_params(m))


@pytest.fixture(scope="module")
def torch_progress_run(world1):
    tr, m, b = _trainer(_graph_cfg("torch"), force_dp=True, progress=True)
    logs = _steps(tr, b, S)
    yield dict(tr=tr, b=b, logs=torch.stack(logs), read=tr.progress.read())
    tr.progress.close()


def _raw(p):
    return [int(p._host[i]) for i in range(p.SLOTS)]


def test_progress_marker_kernel_eager_and_captured():
    """progress_mark_kernel through DeviceProgress: slot 0 counts step marks, slot 1 holds steps * 256 + bucket + 1
    with the count of steps completed BEFORE the step the bucket belongs to; the same marks as graph nodes; the
    255-bucket limit; the C entry point's argument checks."""
    from matcha import _abi
    from matcha import _graphs as G
    from matcha import _native as N
    from matcha.watchdog import DeviceProgress

    def state(steps, bucket, bstep):
        return {"device_steps_done": steps, "device_last_bucket_done": bucket, "device_last_bucket_step": bstep}

    p = DeviceProgress()  # allocates and synchronises: outside any capture
    try:
        assert p.read() == state(0, None, None)
        cur = torch.cuda.current_stream(DEV)
        p.mark_bucket(0, cur)
        p.mark_bucket(4, cur)
        p.mark_step(cur)
        torch.cuda.synchronize()
        assert p.read() == state(1, 4, 0)

        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=G.capture_mode()):  # (its own capturing stream)
            p.mark_bucket(0, torch.cuda.current_stream(DEV))
            p.mark_bucket(2, torch.cuda.current_stream(DEV))
            p.mark_step(torch.cuda.current_stream(DEV))
        torch.cuda.synchronize()
        assert p.read() == state(1, 4, 0)  # capturing ran nothing
        for _ in range(5):
            g.replay()
        torch.cuda.synchronize()
        assert p.read() == state(6, 2, 5)  # replay i marks its buckets with i completed steps: 1 + 4

        assert DeviceProgress.MAX_BUCKETS == 255
        p.mark_bucket(254, cur)
        torch.cuda.synchronize()
        assert p.read() == state(6, 254, 6)
        raw = _raw(p)
        assert raw == [6, 6 * 256 + 255]
        with pytest.raises(ValueError):
            p.mark_bucket(255, cur)
        torch.cuda.synchronize()
        assert _raw(p) == raw

        lib = N.lib()
        for slot, tag in ((p.SLOTS, 1), (p.SLOTS + 5, -1), (-1, 1), (-1, -1), (0, 0), (0, 7), (1, 256)):
            rc = lib.mtts_dp_progress_mark(p._h, slot, tag, cur.cuda_stream)
            assert rc == _abi.MTTS_ERR_INVALID_ARG, (slot, tag, rc)
            assert b"dp_progress_mark" in lib.mtts_last_error(), (slot, tag)
        torch.cuda.synchronize()
        assert _raw(p) == raw
    finally:
        p.close()
        p.close()  # twice is safe
    assert not p._h


def test_captured_dp_step_reports_progress_rccl(rccl_progress_run, rccl_plain_run):
    """The markers as nodes of the step's graph (comm="rccl": after each bucket's all-reduce on the reducer stream,
    at the step's end on the main stream).  Only replays mark: Trainer._graph_capture's two warm-up passes arm the
    reducer pack-only (GradBucketReducer._issue marks only on its overlapped branch), call _clip_and_update
    without the step marker (that call is in the captured closure alone), and the reducer's warm() launches
    all-reduces only -- so S steps read as exactly S.  The markers do not perturb the step."""
    r, r0 = rccl_progress_run, rccl_plain_run
    tr = r["tr"]
    n = len(tr.reducer.buckets)
    assert n >= 3 and tr.reducer.progress is tr.progress
    assert next(iter(tr._graphs.values()))["overlap"] is True
    assert r["read"] == {"device_steps_done": S, "device_last_bucket_done": n - 1, "device_last_bucket_step": S - 1}
    assert torch.equal(r["logs"], r0["logs"]), (r["logs"], r0["logs"])
    for k in r0["params"]:
        assert torch.equal(r["params"][k], r0["params"][k]), k


def test_captured_dp_step_reports_progress_torch(torch_progress_run):
    """comm="torch": the graph only packs, the step marker is launched eagerly after each replayed optimizer graph
    and no bucket is ever marked."""
    r = torch_progress_run
    assert next(iter(r["tr"]._graphs.values()))["overlap"] is False
    assert r["read"] == {"device_steps_done": S, "device_last_bucket_done": None, "device_last_bucket_step": None}
    assert torch.isfinite(r["logs"]).all()


def test_measure_dp_tail_probe_changes_nothing(world1, rccl_progress_run, torch_progress_run):
    """Trainer.measure_dp_tail after 3 captured steps: a well-formed result (no magnitudes: nobody has measured
    this at N>1), and no trace -- parameters, Adam moments, the device step count, the reducer's state -- so that
    the 4th step equals the 4th step of a twin that never probed."""
    from matcha.training import TrainConfig, Trainer

    twin = rccl_progress_run
    tr, m, b = _trainer(_graph_cfg("rccl"), force_dp=True, progress=True)
    try:
        logs = _steps(tr, b, 3)
        assert torch.equal(torch.stack(logs), twin["logs"][:3])
        opt = tr.optimizer
        before = [t.clone() for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_t)]
        params_before = _params(m)
        out = tr.measure_dp_tail([b])
        torch.cuda.synchronize()
        red = tr.reducer
        n = len(red.buckets)
        assert out["tail_bucket"] == n - 1
        assert out["tail_bucket_mb"] == round((red.spans[-1][1] - red.spans[-1][0]) * 4 / 2 ** 20, 3)
        assert math.isfinite(out["tail_pack_allreduce_us"]) and out["tail_pack_allreduce_us"] > 0
        assert math.isfinite(out["tail_exposed_us"]) and out["tail_exposed_us"] >= 0
        for t0, t1 in zip(before, (opt.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_t)):
            assert torch.equal(t0, t1)
        assert float(opt.step_t) == 3.0
        for k, v in _params(m).items():
            assert torch.equal(v, params_before[k]), k
        assert red.tail_events is None
        assert red.armed is False
        # no update happened; the probe's eager pass marked its buckets at 3 completed steps
        assert tr.progress.read() == {"device_steps_done": 3, "device_last_bucket_done": n - 1,
                                      "device_last_bucket_step": 3}
        log4 = _steps(tr, b, 1)[0]
        assert torch.equal(log4, twin["logs"][3]), (log4, twin["logs"][3])
        after = _params(m)
        for k in twin["params"]:
            assert torch.equal(after[k], twin["params"][k]), k
        assert tr.progress.read()["device_steps_done"] == 4
    finally:
        tr.progress.close()
    # only a capturable (RCCL) reducer is probed
    assert torch_progress_run["tr"].measure_dp_tail([torch_progress_run["b"]]) is None
    assert Trainer(_model(12), TrainConfig(graph=True)).measure_dp_tail([b]) is None


def test_eager_bucketed_step_over_rccl_equals_plain_eager_step(world1):
    """dp="buckets", graph=False over RCCL -- the pass measure_dp_tail runs: the recording step, then two steps
    whose all-reduces are forked onto the reducer stream after the deferral's side stream -- against the plain
    eager step.  One-rank ncclSum is the identity and every kernel is fixed-order: bitwise."""
    from matcha.training import TrainConfig

    tr, m, b = _trainer(TrainConfig(graph=False, dp="buckets", comm="rccl", force_dp=True, bucket_mb=4.0))
    logs = torch.stack(_steps(tr, b, 3))
    params = _params(m)
    tr0, m0, b0 = _trainer(TrainConfig(graph=False))
    assert tr0.reducer is None and not tr0.dp
    logs0 = torch.stack(_steps(tr0, b0, 3))
    red = tr.reducer
    assert red is not None and red.comm.capturable and len(red.buckets) >= 3
    assert torch.equal(logs, logs0), (logs, logs0)
    for k, v in _params(m0).items():
        assert torch.equal(params[k], v), k
    # _pack copies exactly the gradients that were not written in place: a gradient of the last armed backward
    # either IS its own flat view (same address; nothing to copy) or lies outside the flat buffer altogether
    lo = red.flat.data_ptr()
    hi = lo + red.flat.numel() * 4
    n_copied = 0
    for k, (s, e) in enumerate(red.buckets):
        want = []
        for i in range(s, e):
            g, v = red.grad_refs[i], red.views[i]
            if lo <= g.data_ptr() < hi:
                assert g.data_ptr() == v.data_ptr() and g.numel() == v.numel(), i
            else:
                want.append(red.params[i].shape)
        assert red.copied[k] == want, k
        n_copied += len(want)
    assert 0 < n_copied < len(red.params)  # both branches of _pack ran
    assert sorted(red.copied) == list(range(len(red.buckets)))


def test_watchdog_reads_a_real_device_object(rccl_progress_run):
    """StepWatchdog(device=DeviceProgress) polling the host-mapped slots while the captured DP steps run: it stays
    quiet (bound 600 s: it cannot fire in this test) and its report names what the device completed."""
    r = rccl_progress_run
    n = len(r["tr"].reducer.buckets)
    assert r["fired"] is False and r["wd_alive"] is False
    for f in (f"device_steps_done={S}", f"device_last_bucket_done={n - 1}", f"device_last_bucket_step={S - 1}"):
        assert f in r["report"], (f, r["report"])
    assert "device=n/a" not in r["report"]
