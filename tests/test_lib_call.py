"""What _lib.call hands to an entry point, without a GPU: a stub in the place of the loaded library records its arguments.  The
stream and the cached workspace belong to a device, so the test supplies both; everything else is the function as it ships."""
import ctypes

import pytest
import torch

from deftet_amd import _lib

STREAM = 0x5EED
CPU = torch.device("cpu")


class _Stub:
    def __init__(self, status=0):
        self.status, self.got = status, None

    def deftet_entry(self, *args):
        self.got = args
        return self.status

    def deftet_last_error(self):
        return b"the stub refused"


@pytest.fixture
def stub(monkeypatch):
    lib = _Stub()
    monkeypatch.setattr(_lib, "_lib", lib)                      # what load() returns once the library is loaded
    monkeypatch.setattr(_lib, "current_stream", lambda device: STREAM)
    return lib


def test_tensors_none_and_host_values(stub):
    a, b = torch.zeros(4), torch.zeros(3, dtype=torch.int64)
    counts = (ctypes.c_int * 2)(5, 6)
    host = 0x1000
    assert _lib.call("deftet_entry", CPU, a, None, b, 7, 0.5, counts, host) is None
    assert stub.got == (a.data_ptr(), None, b.data_ptr(), 7, 0.5, counts, host, STREAM)
    assert all(type(stub.got[i]) is int for i in (0, 2)) and stub.got[5] is counts
    assert len(stub.got) == 8                                   # no workspace pair for an entry that takes none


def test_parameter_is_a_tensor(stub):
    p = torch.nn.Parameter(torch.zeros(2))
    _lib.call("deftet_entry", CPU, p)
    assert stub.got == (p.data_ptr(), STREAM)


def test_workspace_pair_sits_before_the_stream(stub, monkeypatch):
    a = torch.zeros(4)
    own = torch.empty(48, dtype=torch.uint8)
    _lib.call("deftet_entry", CPU, a, 3, ws=own)                # the caller's buffer
    assert stub.got == (a.data_ptr(), 3, own.data_ptr(), 48, STREAM)
    _lib.call("deftet_entry", CPU, a, 3, ws=None)               # (NULL, 0)
    assert stub.got == (a.data_ptr(), 3, None, 0, STREAM)
    cached, asked = torch.empty(4096, dtype=torch.uint8), []
    monkeypatch.setattr(_lib, "workspace", lambda device, nbytes: asked.append((device, nbytes)) or cached)
    _lib.call("deftet_entry", CPU, a, 3, ws=100)                # a byte count: the cached buffer and ITS size
    assert asked == [(CPU, 100)]
    assert stub.got == (a.data_ptr(), 3, cached.data_ptr(), 4096, STREAM)
    _lib.call("deftet_entry", CPU, a, 3, ws=0)                  # zero bytes asked for is still a workspace, not `None`
    assert asked[-1] == (CPU, 0) and stub.got[2:4] == (cached.data_ptr(), 4096)


def test_status_raises_with_the_last_error(stub):
    stub.status = -1
    with pytest.raises(_lib.DefTetHipError) as e:
        _lib.call("deftet_entry", CPU, 1)
    assert str(e.value) == "deftet_entry failed (-1): the stub refused"
    with pytest.raises(_lib.DefTetHipError) as e:
        _lib.call("deftet_entry", CPU, 1, what="deftet_entry(count)")
    assert str(e.value) == "deftet_entry(count) failed (-1): the stub refused"


def test_unknown_entry_is_an_error(stub):
    with pytest.raises(AttributeError):
        _lib.call("deftet_no_such_entry", CPU)
