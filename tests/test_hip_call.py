"""CPU: _hip.call, the one way the operator wrappers reach an entry point whose last parameter is the stream
(retinanet_mi355x/_hip.py).  The library, the device guard and the stream query are replaced here, so what the C side would
receive, and when the stream is read, is checked without a GPU."""
import types

import pytest
import torch


@pytest.fixture
def fake(monkeypatch):
    from retinanet_mi355x import _hip
    log = types.SimpleNamespace(calls=[], guards=[], inside=[], stream_read_inside=[], rc=0)

    class Lib:
        def __getattr__(self, name):
            def fn(*args):
                log.calls.append((name, args))
                return log.rc
            return fn

    class Guard:
        def __init__(self, device):
            self.device = device

        def __enter__(self):
            log.guards.append(self.device)
            log.inside.append(self.device)

        def __exit__(self, *exc):
            log.inside.pop()

    def current_stream(device=None):
        log.stream_read_inside.append(list(log.inside))
        return types.SimpleNamespace(cuda_stream=0x5EED)

    monkeypatch.setattr(_hip, "load", lambda: Lib())
    monkeypatch.setattr(torch.cuda, "device", Guard)
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    return log


def test_tensors_pass_their_pointer_and_none_stays_none(fake):
    from retinanet_mi355x import _hip
    a, b = torch.zeros(6), torch.zeros(3, dtype=torch.int32)
    assert _hip.call("rn_x", a, None, 7, 0.5, b[1:]) is None
    (name, args), = fake.calls
    assert name == "rn_x"
    assert args[:5] == (a.data_ptr(), None, 7, 0.5, b.data_ptr() + 4)
    assert type(args[2]) is int and type(args[3]) is float          # scalars go as given


def test_an_empty_tensor_or_view_passes_null(fake):
    from retinanet_mi355x import _hip
    full = torch.zeros((4, 6))
    assert full.data_ptr() != 0
    _hip.call("rn_x", full[2:2], full[:, :0], torch.zeros(0), torch.empty((0, 4), dtype=torch.float64))
    assert fake.calls[0][1][:4] == (0, 0, 0, 0)


def test_the_stream_goes_last_and_is_read_inside_the_guard(fake):
    from retinanet_mi355x import _hip
    _hip.call("rn_x", 1, 2, device="cuda:3")
    assert fake.calls[0][1] == (1, 2, 0x5EED)
    assert fake.guards == ["cuda:3"] and fake.stream_read_inside == [["cuda:3"]] and fake.inside == []


def test_without_a_device_no_guard_is_entered(fake):
    from retinanet_mi355x import _hip
    _hip.call("rn_x", 1)
    _hip.call("rn_y")
    assert fake.calls == [("rn_x", (1, 0x5EED)), ("rn_y", (0x5EED,))]
    assert fake.guards == [] and fake.stream_read_inside == [[], []]


@pytest.mark.parametrize("device", [None, "cuda:0"])
def test_a_return_code_raises_with_the_symbol_and_the_error_name(fake, device):
    from retinanet_mi355x import _hip
    for rc, text in sorted(_hip.RN_ERRORS.items()) + [(719, "hipError_t 719")]:
        fake.rc = rc
        with pytest.raises(RuntimeError) as e:
            _hip.call("rn_some_entry", torch.zeros(1), device=device)
        assert str(e.value) == "rn_some_entry failed: " + text
    assert _hip.RN_ERRORS[10001].startswith("RN_EINVAL") and _hip.RN_ERRORS[10002].startswith("RN_ETOOMANY")
    assert fake.inside == []                                          # the guard is left on the way out
