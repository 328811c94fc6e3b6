"""The poison-and-guard helper (tests/poison.py) must FAIL when it should: pure-torch stand-in "ops" on the CPU with each of the
mistakes the GPU cases of tests/test_gpu_47_poisoned_memory.py look for -- an unwritten element, a store past either end of an
output, a workspace word read before it is written -- and a correct op that passes with unchanged bits."""
import pytest
import torch

from tests import poison


@pytest.fixture(autouse=True)
def _cpu_poison(monkeypatch):
    monkeypatch.setattr(poison, "POISON_CPU", True)


def _run(op, x, int_bodies=True):
    """The harness of the GPU cases in small: once unpatched, once poisoned; guards checked on exit."""
    plain = op(x)
    with poison.poisoned_allocations(int_bodies, name=op.__name__):
        got = op(x)
    return plain, got


def _assert_clean(got):
    for k, t in got.items():
        assert not bool(poison.holds_poison(t).any()), f"poison in result {k}"


# ---- the stand-in ops ------------------------------------------------------------------------------------------------------------
def op_correct(x):
    out = torch.empty(x.shape[0], 3)
    ws = x.new_empty((x.shape[0],), dtype=torch.int32)
    ws.copy_((x > 0).to(torch.int32))
    idx = torch.empty_like(ws, dtype=torch.int64)
    idx.copy_(torch.cumsum(ws, 0))
    out.copy_(torch.stack([x, x * 2, x + idx.float()], 1))
    flags = torch.empty(x.shape[0], dtype=torch.bool)
    flags.copy_(x > 0)
    return {"out": out, "idx": idx, "flags": flags}


def op_writes_half(x):
    out = torch.empty(x.shape[0])
    out[: x.shape[0] // 2] = x[: x.shape[0] // 2] * 2
    return {"out": out}


def op_writes_one_past_the_end(x):
    out = torch.empty(x.shape[0])
    wide = out.as_strided((x.shape[0] + 1,), (1,), out.storage_offset())      # the returned view's storage, one element more
    wide[:-1] = x
    wide[-1] = 1.0
    return {"out": out}


def op_writes_one_before_the_start(x):
    out = torch.empty(x.shape[0], dtype=torch.int32)
    wide = out.as_strided((x.shape[0] + 1,), (1,), out.storage_offset() - 1)
    wide[1:] = x.to(torch.int32)
    wide[0] = 7
    return {"out": out}


def op_reads_workspace_before_writing(x):
    counts = torch.empty(4, dtype=torch.int32)          # a "count slot" the op accumulates into without clearing it first
    counts += torch.bincount((x > 0).long(), minlength=4).to(torch.int32)
    return {"counts": counts}


# ---- the self-tests --------------------------------------------------------------------------------------------------------------
X = torch.linspace(-1.0, 1.0, 37)


def test_unwritten_half_is_reported_as_poison_in_result():
    _, got = _run(op_writes_half, X)
    with pytest.raises(AssertionError, match="poison in result out"):
        _assert_clean(got)
    bad = poison.holds_poison(got["out"])
    assert not bool(bad[:18].any()) and bool(bad[18:].all())
    # ... also when the unwritten element is an integer, with the integer poison on
    with poison.poisoned_allocations(True):
        t = torch.empty(5, dtype=torch.int32)
        t[:4] = 1
    assert poison.holds_poison(t).tolist() == [False] * 4 + [True] and int(t[4]) == 2139062143
    with poison.poisoned_allocations(False):
        t = torch.empty(5, dtype=torch.int64)
    assert t.tolist() == [0] * 5


def test_write_past_the_end_is_reported_with_site_and_offset():
    with pytest.raises(poison.GuardViolation) as e:      # (poisoned only: unpatched, the storage ends with the output)
        with poison.poisoned_allocations(True):
            op_writes_one_past_the_end(X)
    (v,) = e.value.violations
    assert v["side"] == "back" and v["offset"] == 37 * 4 and v["nbytes"] == 37 * 4
    assert "test_poison_helper.py" in v["site"] and v["site"].endswith("in op_writes_one_past_the_end")
    line = int(v["site"].split(":")[-1].split(" ")[0])
    assert line == op_writes_one_past_the_end.__code__.co_firstlineno + 1
    assert "op_writes_one_past_the_end" in str(e.value) and "+148" in str(e.value)


def test_write_before_the_start_is_reported_with_site_and_offset():
    with pytest.raises(poison.GuardViolation) as e:
        with poison.poisoned_allocations(True):
            op_writes_one_before_the_start(X)
    (v,) = e.value.violations
    assert v["side"] == "front" and v["offset"] == -4 and v["dtype"] == "int32"
    assert v["site"].endswith("in op_writes_one_before_the_start")


def test_read_before_write_changes_the_result_and_bit_equality_catches_it():
    plain = {"counts": torch.bincount((X > 0).long(), minlength=4).to(torch.int32)}      # what the op means to return
    with poison.poisoned_allocations(True):
        got = op_reads_workspace_before_writing(X)
    assert not torch.equal(got["counts"], plain["counts"])
    # with zeroed integer bodies the mistake hides: that is what ``int_bodies`` is for
    with poison.poisoned_allocations(False):
        hidden = op_reads_workspace_before_writing(X)
    assert torch.equal(hidden["counts"], plain["counts"])


def test_correct_op_passes_with_unchanged_bits():
    plain, got = _run(op_correct, X)
    _assert_clean(got)
    assert set(plain) == set(got)
    for k in plain:
        assert plain[k].dtype == got[k].dtype and plain[k].shape == got[k].shape and got[k].is_contiguous()
        assert torch.equal(plain[k], got[k]), k
        assert got[k]._base is None and got[k].data_ptr() % 64 == 0


def test_the_real_functions_are_back_after_the_context():
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with poison.poisoned_allocations(True):
        assert torch.empty is not real[0] and torch.empty_like is not real[1] and torch.Tensor.new_empty is not real[2]
    assert torch.empty is real[0] and torch.empty_like is real[1] and torch.Tensor.new_empty is real[2]
    with pytest.raises(ZeroDivisionError):
        with poison.poisoned_allocations(True):
            1 / 0
    assert torch.empty is real[0] and torch.empty_like is real[1] and torch.Tensor.new_empty is real[2]


def test_layout_of_a_poisoned_buffer_and_the_pass_through_calls():
    with poison.poisoned_allocations(True) as pz:
        a = torch.empty(3, 5)
        b = torch.empty((2, 0, 4), dtype=torch.float64)
        c = torch.empty(7, dtype=torch.uint8)
        d = torch.empty_like(a.t())                       # non-contiguous, preserve_format: passed through
        e = torch.empty(4, dtype=torch.float16)           # a dtype the helper does not know: passed through
        f = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        g = a.new_empty(6)
        h = torch.empty(3, out=torch.zeros(3))
        assert len(pz.records) == 4
    assert a.shape == (3, 5) and a.stride() == (5, 1) and a.storage_offset() == poison.GUARD_BYTES // 4
    assert bool(poison.holds_poison(a).all()) and bool(torch.isnan(a).all())
    assert int(a.view(torch.int32)[0, 0]) == 0x7FC0BD5A
    assert b.numel() == 0 and b.shape == (2, 0, 4)
    assert c.tolist() == [0x7F] * 7
    assert d.stride() == (1, 5) and e.dtype == torch.float16 and f.is_contiguous(memory_format=torch.channels_last)
    assert g.shape == (6,) and bool(poison.holds_poison(g).all()) and h.shape == (3,)
    x64 = torch.empty(0, dtype=torch.float64)
    with poison.poisoned_allocations(True):
        x64 = torch.empty(2, dtype=torch.float64)
    assert x64.view(torch.int64).tolist() == [poison.F64_POISON] * 2 and bool(torch.isnan(x64).all())


def test_gpu_fault_text_is_recognised():
    assert poison.is_gpu_fault(RuntimeError("HIP error: an illegal memory access was encountered"))
    assert not poison.is_gpu_fault(RuntimeError("bds_ssim_fwd failed: invalid argument (code -1)"))
