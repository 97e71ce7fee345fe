"""CPU: the runtime plumbing every native-backed model inherits from native_model.NativeModel — what travels with a pickle or
a deepcopy, what a train()/eval() switch, load_state_dict() and a dtype / device move drop, the token-table switch and the
row-limit scope — on the six model classes with a tiny configuration.  Nothing here touches the HIP library."""
import copy
import pickle

import pytest
import torch

from show_edit_tell_amd import _lib, dcnet, dcnet_rl, dcnet_with_mse, editnet, editnet_adaptive, editnet_rl
from show_edit_tell_amd.native_model import NativeModel

WM = {"<pad>": 0, "<start>": 1, "<end>": 2, "<unk>": 3, "a": 4, "b": 5, "c": 6}
D = 64
EDITNET = (editnet.DecoderC, editnet_rl.DecoderC, editnet_adaptive.DecoderC)
DCNET = (dcnet.DAE, dcnet_rl.DAE, dcnet_with_mse.DAE)
CLASSES = EDITNET + DCNET
IDS = [c.__module__.rsplit(".", 1)[1] + "." + c.__name__ for c in CLASSES]


def make(cls):
    torch.manual_seed(0)
    if cls in EDITNET:
        return cls(WM, decoder_dim=D, caption_features_dim=D, emb_dim=D, attention_dim=32, image_features_dim=48)
    return cls(WM, None, decoder_dim=D, attention_dim=32, caption_features_dim=D, emb_dim=D)


def plant(m):
    """a dummy value under every runtime attribute name"""
    for k in NativeModel._RUNTIME_ATTRS:
        m.__dict__[k] = {"dummy": k}
    return m


def assert_clean(m):
    left = [k for k in NativeModel._RUNTIME_ATTRS if k in m.__dict__ and k not in ("_ws", "_ws_key")]
    assert not left, left
    assert m._ws is None and m._ws_key is None


def test_every_model_takes_the_plumbing_from_the_one_base():
    for cls in CLASSES:
        assert issubclass(cls, NativeModel) and cls._RUNTIME_ATTRS is NativeModel._RUNTIME_ATTRS
        assert cls.row_limits is None and cls._ABI in ("editnet", "dcnet")
        for name in ("__getstate__", "invalidate_token_table", "train", "load_state_dict", "_apply", "init_hidden_state",
                     "_grad_path", "_weights", "_token_table", "_workspace", "_new_workspace", "ws_tensor", "_row_limits_scope"):
            assert getattr(cls, name) is getattr(NativeModel, name), (cls, name)


@pytest.mark.parametrize("cls", CLASSES, ids=IDS)
def test_pickle_and_deepcopy_drop_the_runtime_state(cls):
    m = plant(make(cls))
    keys = list(m.state_dict().keys())
    for back in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert type(back) is cls
        assert_clean(back)
        assert list(back.state_dict().keys()) == keys
        assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), m.state_dict().values()))
        if cls in DCNET:                                    # the weakref to the owner is restored, to the COPY
            assert back.caption_encoder._owner() is back
    assert all(k in m.__dict__ for k in NativeModel._RUNTIME_ATTRS), "the original keeps its runtime state"
    assert set(m.__getstate__()) == set(make(cls).__dict__), "a pickle holds what a fresh module holds, no more"


@pytest.mark.parametrize("cls", CLASSES, ids=IDS)
def test_mode_switches_and_loads_drop_the_token_table(cls):
    m = make(cls)
    assert m.training
    plant(m).eval()                                         # train -> eval
    assert "_tok_state" not in m.__dict__ and "_ws_cache" in m.__dict__
    plant(m).eval()                                         # eval on an eval module keeps the table
    assert m.__dict__["_tok_state"] == {"dummy": "_tok_state"}
    m.train(False)
    assert "_tok_state" in m.__dict__
    m.train()                                               # eval -> train
    assert "_tok_state" not in m.__dict__
    plant(m).train()                                        # train on a training module keeps it too
    assert "_tok_state" in m.__dict__
    m.load_state_dict(m.state_dict())
    assert "_tok_state" not in m.__dict__ and "_ws_cache" in m.__dict__
    plant(m).invalidate_token_table()
    assert "_tok_state" not in m.__dict__


@pytest.mark.parametrize("cls", CLASSES, ids=IDS)
def test_a_dtype_or_device_move_drops_tables_workspaces_and_prologues(cls):
    m = plant(make(cls))
    assert m.float() is m
    for k in ("_tok_state", "_ws_cache", "_ahead", "_ahead_free", "_grad_buckets"):
        assert k not in m.__dict__, k
    assert m._ws is None and m._ws_key is None
    assert m.__dict__["_fwd_seed"] == {"dummy": "_fwd_seed"}            # (what does not hold device memory stays)


def test_dae_with_ar_takes_a_stage_one_dae_over():
    dae = make(dcnet.DAE)
    keys = list(dae.state_dict().keys())
    wrapped = dcnet_with_mse.DAEWithAR(dae=dae)
    assert wrapped.dae is dae and type(dae) is dcnet_with_mse.DAE and isinstance(dae, NativeModel)
    assert list(dae.state_dict().keys()) == keys and dae.caption_encoder._owner() is dae
    assert dcnet_with_mse.DAEWithAR(dae=make(dcnet_with_mse.DAE)).dae.__class__ is dcnet_with_mse.DAE
    with pytest.raises(TypeError):
        dcnet_with_mse.DAEWithAR(dae=make(editnet.DecoderC))


@pytest.mark.parametrize("cls", CLASSES, ids=IDS)
def test_token_table_switched_off_never_loads_the_library(cls, monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    monkeypatch.setenv("SET_TOKEN_TABLE", "0")
    m = make(cls).eval()
    dims = m._dims(2, 5, 7, 19) if cls in EDITNET else m._dims(2, 5, 19)
    assert m._token_table_supported(dims) == (cls in EDITNET)           # D = 64; DCNet also wants C % 128 == 0
    assert len(m._token_table_sources()) == 6
    for _ in range(3):
        assert m._token_table(dims) is None
    assert "_tok_state" not in m.__dict__
    monkeypatch.setenv("SET_TOKEN_TABLE", "1")
    if cls in DCNET:                                                    # unsupported dims: no table, no library either
        assert m._token_table(dims) is None and "_tok_state" not in m.__dict__


class _StubLib:
    def __init__(self):
        self.calls = []

    def set_decode_row_limits(self, p):
        self.calls.append(p)
        return 0


class _FakeLimits:
    """stands in for a device tensor (this test has no GPU): what _row_limits_scope looks at, and a pointer"""
    dtype, is_cuda = torch.int32, True

    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n

    def contiguous(self):
        return self

    def data_ptr(self):
        return 0x1000


@pytest.mark.parametrize("cls", CLASSES, ids=IDS)
def test_row_limits_scope(cls):
    m = make(cls)
    lib = _StubLib()
    with m._row_limits_scope(lib, 3):                       # no limits: the pointer is cleared on entry, nothing on exit
        assert lib.calls == [None]
    assert lib.calls == [None]
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), _FakeLimits(4)):
        m.row_limits = bad                                  # wrong dtype / a CPU tensor / a wrong length
        lib = _StubLib()
        with pytest.raises(_lib.SetError, match="row_limits must be an int32 device tensor with one entry per row"):
            with m._row_limits_scope(lib, 3):
                raise AssertionError("entered")
        assert lib.calls == []
    m.row_limits = _FakeLimits(3)
    lib = _StubLib()
    with pytest.raises(KeyError):                           # set on entry, cleared on exit — on an exception too
        with m._row_limits_scope(lib, 3):
            assert len(lib.calls) == 1 and lib.calls[0].value == 0x1000
            raise KeyError("inside")
    assert len(lib.calls) == 2 and lib.calls[1] is None
    assert type(m).row_limits is None, "the limits are the instance's"
