"""GPU: the data-parallel overlap probe (pdvc/step_graph.py dp_overlap_supported) tells a gating event from one that
does not gate, deterministically: with the side stream's wait made a no-op, the waiting copy runs while
the probe's replay is held at its host flag, and the probe must answer False every time; with the real wait, True.

Which hardware queue a stream of torch's pool lands on depends on what the process ran before, and a side stream on
the replay's own queue cannot run beside it (the probe then keeps the serial reduction, rightly, and there is nothing
to tell apart).  So the test first picks a pool stream that does run while a replayed graph holds the default stream
(`stream_beside_a_held_replay`) and hands the probe that one: every assertion below is then checked in every run."""
import ctypes
import time

import pytest
import torch

pytestmark = pytest.mark.gpu


def stream_beside_a_held_replay():
    """A stream of torch's pool whose work completes while a graph replay on the default stream is held at a host flag
    (the probe's own gate, pdvc_spin_until_flag, bounded at 5 s), or None when all 32 pool streams wait behind it."""
    from pdvc import _native as _n
    host, dev = ctypes.c_void_p(), ctypes.c_void_p()
    _n.call("pdvc_host_flag_alloc", ctypes.byref(host), ctypes.byref(dev))
    flag = ctypes.c_int.from_address(host.value)
    found = None
    try:
        mark = torch.zeros(1, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _n.call("pdvc_spin_until_flag", dev, 1, 5000, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            mark.fill_(1.0)
        flag.value = 0
        torch.cuda.synchronize()
        g.replay()
        for _ in range(32):
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                seen = mark.clone()
                done = torch.cuda.Event()
                done.record()
            t0 = time.time()
            while not done.query() and time.time() - t0 < 0.05:
                time.sleep(0.001)
            if done.query():
                found = s
                break
        flag.value = 1
        torch.cuda.synchronize()
        if found is not None:
            assert float(seen) == 0.0, "the picked stream ran ahead of the held replay's write"
        del g
    finally:
        flag.value = 1
        torch.cuda.synchronize()
        _n.call("pdvc_host_flag_free", host)
    return found


def test_probe_rejects_a_wait_that_does_not_hold(monkeypatch):
    from pdvc import distributed as D
    from pdvc import step_graph as SG
    monkeypatch.delenv("PDVC_DP_OVERLAP", raising=False)
    side = stream_beside_a_held_replay()
    if side is None:
        pytest.skip("needs a second hardware queue: no stream of the pool runs beside a held graph replay here")
    saved = list(SG._DP_OVERLAP)
    try:
        for _ in range(3):
            SG._DP_OVERLAP.clear()
            SG._DP_TRIALS.clear()
            with monkeypatch.context() as m:
                m.setattr(D.GraphEvent, "wait", lambda self, stream: None)
                assert SG.dp_overlap_supported(side) is False
            # the side stream ran beside the held replay: the unheld copy read the replay's zero marker
            assert SG._DP_TRIALS and all(c for c, *_ in SG._DP_TRIALS), SG._DP_TRIALS
            assert all(vc == 0.0 and v == 0.0 for _, _, vc, v in SG._DP_TRIALS), SG._DP_TRIALS
        SG._DP_OVERLAP.clear()
        SG._DP_TRIALS.clear()
        ok = SG.dp_overlap_supported(side)
        assert SG._DP_TRIALS and all(c for c, *_ in SG._DP_TRIALS), SG._DP_TRIALS
        assert ok is True, SG._DP_TRIALS
        assert all(h and v in (7.0, 3.0) for _, h, _, v in SG._DP_TRIALS)
    finally:
        SG._DP_OVERLAP[:] = saved
