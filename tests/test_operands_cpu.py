"""CPU: the table of `operand_cases.py` against `ops`, the device guard of the wrappers, and the stub library.

No GPU: the census reads signatures, `_on_operand_device` is driven with stand-ins for tensors, and the stub is asked for its entry
points without calling one that launches.
"""
import ctypes

import pytest
import torch

import operand_cases as oc
from frmap_amd import _lib, ops


def test_census_covers_every_tensor_taking_wrapper():
    found = oc.census()
    assert len(found) >= 40 and "verify_counts" in found and "match_radius" in found and "MatchPack" in found
    # the written operands the issue names, and no row without a valid call
    assert {r.name: r.writes for r in oc.ROWS if r.writes} == {
        "classify_tally": ("state",), "track_step": ("state",), "track_fuse": ("state",), "ovr_append": ("store", "store_labels"),
        "match_top1": ("packed",), "gap_norm_match": ("packed",)}
    for row in oc.ROWS:
        values = row.build()
        assert set(row.tensors) <= set(values), (row.name, sorted(set(row.tensors) - set(values)))
        assert all(isinstance(values[n], torch.Tensor) for n in row.tensors), row.name
        row.signature().bind(**values)                                  # the valid call is a call of this wrapper


def test_every_dependent_operand_has_its_defects():
    cases = oc.dependent_cases()
    assert len(oc.dependent_pairs()) >= 60 and len(cases) >= 5 * len(oc.dependent_pairs()) - 4      # (`at_least` rules: no "long")
    for row, operand in oc.dependent_pairs():
        valid = row.build()[operand]
        made = oc.defects(row, operand, valid)
        assert [m[0] for m in made] == oc.DEFECT_LABELS[(row.name, operand)]
        for label, bad, exc in made:
            if label.startswith("short"):
                assert bad.numel() < valid.numel() and bad.dim() == valid.dim() and exc is ValueError
            elif label.startswith("long"):
                assert bad.numel() > valid.numel() and bad.dim() == valid.dim() and exc is ValueError
            elif label == "rank":
                assert bad.numel() == valid.numel() and bad.dim() != valid.dim() and exc is ValueError
            elif label == "dtype":
                assert bad.dtype != valid.dtype and bad.shape == valid.shape and exc is TypeError
            else:
                assert label == "cpu" and isinstance(bad, oc._OnCpu) and exc is RuntimeError


@pytest.mark.parametrize("wrapper,extent,file,fragment", oc.own_citations(), ids=["%s-%s" % (c[0], c[1].split(" ")[0]) for c in oc.own_citations()])
def test_an_extent_left_to_the_library_cites_the_check_that_refuses_it(wrapper, extent, file, fragment):
    line = oc.citation_line(file, fragment)
    assert line is not None and "FRMAP_REQUIRE(" in line, (wrapper, extent, file, fragment)


def test_every_row_launches_on_its_operands_device():
    """The registration loop at the end of the wrappers: nobody is left out (`verify_counts` and `match_radius` once were)."""
    missing = []
    for row in oc.ROWS:
        fn = row.target().__init__ if isinstance(row.target(), type) else row.target()
        if not callable(getattr(fn, "__wrapped__", None)):
            missing.append(row.name)
    assert missing == []
    assert callable(getattr(ops.MatchPack.update_rows, "__wrapped__", None))


# ---------------------------------------------------------------------------------------------------------------------------------
# `_on_operand_device` itself, on stand-ins
# ---------------------------------------------------------------------------------------------------------------------------------
class _Dev:
    def __init__(self, index):
        self.index = index

    def __eq__(self, other):
        return isinstance(other, _Dev) and other.index == self.index

    def __ne__(self, other):
        return not self == other

    def __repr__(self):
        return "cuda:%d" % self.index


class _Tensor(torch.Tensor):
    """A tensor that says it lives on a GPU (`is_cuda`, `device`): all `_on_operand_device` asks of an operand."""
    @staticmethod
    def on(index, cuda=True):
        t = torch.zeros(1).as_subclass(_Tensor)
        t._dev, t._cuda = _Dev(index), cuda
        return t

    @property
    def is_cuda(self):
        return self._cuda

    @property
    def device(self):
        return self._dev


class _Cuda:
    """`torch.cuda` as far as the guard uses it: the current device, and the context manager that changes it."""

    def __init__(self):
        self.current, self.entered = 0, []

    def current_device(self):
        return self.current

    def device(self, dev):
        outer = self

        class Ctx:
            def __enter__(self):
                self.saved, outer.current = outer.current, dev.index
                outer.entered.append(dev.index)

            def __exit__(self, *exc):
                outer.current = self.saved
        return Ctx()


class _Torch:
    Tensor = torch.Tensor

    def __init__(self):
        self.cuda = _Cuda()


@pytest.fixture
def fake(monkeypatch):
    t = _Torch()
    monkeypatch.setattr(ops, "torch", t)
    seen = []

    @ops._on_operand_device
    def fn(*args, **kwargs):
        seen.append(t.cuda.current)
        return "ran"
    return fn, t.cuda, seen


def _pack_on(index):
    pack = object.__new__(ops.MatchPack)                 # (no constructor: it would launch)
    pack.packed = _Tensor.on(index)
    return pack


def test_the_guard_sees_positional_keyword_and_prepared_operands(fake):
    fn, cuda, seen = fake
    assert fn(_Tensor.on(0), 3) == "ran" and cuda.entered == [] and seen == [0]                  # the current device: nothing to enter
    assert fn(_Tensor.on(1)) == "ran" and cuda.entered == [1] and seen[-1] == 1 and cuda.current == 0
    assert fn(2.5, b=_Tensor.on(1)) == "ran" and cuda.entered == [1, 1] and seen[-1] == 1       # by keyword only (match_radius' b=)
    assert fn(prepared=_pack_on(1)) == "ran" and cuda.entered == [1, 1, 1] and seen[-1] == 1    # inside a MatchPack
    assert fn(_Tensor.on(1), labels_a=_Tensor.on(1), prepared=_pack_on(1), which="all") == "ran" and seen[-1] == 1
    assert fn(_Tensor.on(1, cuda=False), 7) == "ran" and seen[-1] == 0                           # a CPU tensor decides nothing (`_dev` refuses it)
    assert fn() == "ran" and seen[-1] == 0


def test_the_guard_refuses_operands_on_two_devices(fake):
    fn, cuda, seen = fake
    for args, kwargs in [((_Tensor.on(0), _Tensor.on(1)), {}), ((_Tensor.on(0),), {"b": _Tensor.on(1)}),
                         ((), {"labels_a": _Tensor.on(1), "labels_b": _Tensor.on(0)}), ((_Tensor.on(0),), {"prepared": _pack_on(1)})]:
        with pytest.raises(ValueError, match="different devices"):
            fn(*args, **kwargs)
    assert seen == [] and cuda.entered == []


# ---------------------------------------------------------------------------------------------------------------------------------
# the stub
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_stub_forwards_exactly_the_pointer_free_prototypes(monkeypatch):
    real = _lib.load()
    stub = oc.install(monkeypatch)
    assert _lib.load() is stub
    free = set(oc.pointer_free())
    pointer_types = (ctypes.c_void_p, ctypes.c_char_p)
    for name, (_, argtypes) in _lib.PROTOTYPES.items():
        takes_pointer = any(a in pointer_types or hasattr(a, "contents") for a in argtypes)         # (POINTER(c_float) has `contents`)
        assert (name in free) == (not takes_pointer), name
        fn = getattr(stub, name)
        if name in free:
            assert fn is getattr(real, name) or fn == getattr(real, name), name
        else:
            before = len(stub.calls)
            with pytest.raises(oc.ReachedLibrary) as e:
                fn(*range(len(argtypes)))
            assert e.value.entry == name and stub.calls[before:] == [(name, tuple(range(len(argtypes))))]
    # what the wrappers ask before they launch is answered by the real library ...
    for name in ("frmap_linear_mfma_workspace_bytes", "frmap_match_workspace_bytes", "frmap_head_workspace_bytes", "frmap_match_topk_workspace_bytes",
                 "frmap_verify_workspace_bytes", "frmap_match_radius_workspace_bytes", "frmap_conv_igemm_pool2_supported",
                 "frmap_conv_igemm_ds_supported", "frmap_small_cin_kpad", "frmap_last_error", "frmap_classify_tally_words",
                 "frmap_track_state_bytes", "frmap_track_fuse_state_bytes"):
        assert name in free, name
    assert stub.frmap_small_cin_kpad(3, 3) == real.frmap_small_cin_kpad(3, 3) > 0
    assert ops.classify_tally_words(5) == int(real.frmap_classify_tally_words(5, 6, 10, 1))     # (through `ops`, through the stub)
    # ... and nothing that takes memory is: every launching entry point of the alignment table, and every host twin
    assert not free & set(_lib.ALIGNMENT) and not {n for n in _lib.PROTOTYPES if n.endswith("_host")} & free
    with pytest.raises(AttributeError):
        stub.frmap_no_such_entry
    monkeypatch.undo()
    assert _lib.load() is real
