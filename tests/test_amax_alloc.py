"""CPU: which zeroed chunk the split3 amax words come from (retinanet_mi355x/conv.py: _amax_chunk_key / _amax_alloc).

A chunk made while a graph is being captured is zeroed by a fill that only THAT graph replays; an eager chunk is zeroed once.  So two
captures must never slice one chunk, and eager work and a capture must never share one -- or the exponent bytes of one replay survive
into the next (tests/test_gpu_amax.py shows what that does to the results).  The stream and capture queries are replaced here, so the
rule is checked without a GPU."""
import types

import pytest
import torch


@pytest.fixture
def fake(monkeypatch):
    from retinanet_mi355x import conv
    state = {"stream": 7, "capture": 0}
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=state["stream"]))
    monkeypatch.setattr(conv, "capture_id", lambda stream: state["capture"] if stream == state["stream"] else 0)
    monkeypatch.setattr(conv, "_AMAX_CHUNK", {})
    held = []                                          # the words stay referenced: no storage is freed and its address reused

    def chunk(stream, capture):
        state["stream"], state["capture"] = stream, capture
        words = conv.amax_slot("cpu", 2)
        assert words.numel() == 2 * conv.AMAX_SUB and int(words.abs().sum()) == 0
        held.append(words)
        return words.untyped_storage().data_ptr()
    chunk.table = lambda: conv._AMAX_CHUNK
    return chunk


def test_two_captures_on_one_stream_never_share_a_chunk(fake):
    first = fake(7, 101)
    assert fake(7, 101) == first                       # one capture: slices of one chunk (zeroed once per replay)
    second = fake(7, 102)                              # torch.cuda.graph captures every graph on the same stream
    assert second != first
    assert fake(7, 102) == second


def test_eager_and_captured_allocations_never_share_a_chunk(fake):
    eager = fake(9, 0)
    captured = fake(9, 201)                            # a capture on a stream that ran eagerly before
    assert captured != eager
    assert fake(9, 0) == eager                         # eager work after the capture: back on the eager chunk
    assert fake(9, 202) not in (eager, captured)
    assert fake(3, 0) != eager                         # and per stream, as before


def test_the_default_stream_is_never_asked_and_finished_captures_are_let_go(fake, monkeypatch):
    from retinanet_mi355x import conv
    fake(5, 301)
    fake(6, 401)                                       # another stream's capture
    fake(5, 0)
    assert [k[1:] for k in fake.table()] == [(6, 401), (5, 0)]     # stream 5's finished capture dropped, stream 6's kept
    fake(5, 302)
    assert sorted(k[1:] for k in fake.table()) == [(5, 0), (5, 302), (6, 401)]
    monkeypatch.setattr(conv, "capture_id", lambda stream: pytest.fail("capture query on the legacy default stream"))
    fake(0, 0)
