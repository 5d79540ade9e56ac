"""The guarded-operand helper on CPU tensors: view placement, guard detection of a planted write, dense()."""
import pytest
import torch

import guarded as G


@pytest.mark.parametrize("dtype,per16", [(torch.float32, 4), (torch.bfloat16, 8), (torch.int32, 4), (torch.uint8, 16)])
def test_strided_placement(dtype, per16):
    rows, width = 7, 36
    data = (torch.arange(rows * width).reshape(rows, width) % 100).to(dtype)
    g = G.strided_in(data, device="cpu", int_guard=0x7FFFFFFF if dtype == torch.int32 else 255)
    assert g.ld == g.view.stride(0) and g.ld > width and g.view.stride(1) == 1
    assert g.origin == (G.GUARD_ROWS, per16) and g.buf.shape[0] == rows + 2 * G.GUARD_ROWS
    off = g.view.data_ptr() - g.buf.data_ptr()
    assert off == (G.GUARD_ROWS * g.ld + per16) * data.element_size() and off % 16 == 0 and off % 64 != 0
    assert torch.equal(G.dense(g.view), data) and G.dense(g.view).is_contiguous()
    if dtype.is_floating_point:                  # NaN everywhere around the data
        m = g._mask()
        assert bool(torch.isnan(g.buf.float()[m]).all()) and not bool(torch.isnan(g.view.float()).any())


def test_explicit_odd_stride():
    g = G.strided_out(5, 30, ld=35, device="cpu")
    assert g.ld == 35 and g.view.shape == (5, 30)
    h = G.strided_out(5, 30, ld=34, device="cpu")        # smallest stride: the next row's left guard follows a row's end
    h.buf.view(-1)[(G.GUARD_ROWS + 1) * 34 + 4 + 30] = 1.0   # one element past the end of row 1
    with pytest.raises(AssertionError) as e:
        h.check("planted")
    assert "(row 2, column -4)" in str(e.value)
    with pytest.raises(AssertionError):
        G.strided_out(5, 30, ld=33, device="cpu")        # the view does not fit


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32, torch.uint8])
def test_output_guard_detects_planted_writes(dtype):
    rows, width = 5, 24
    g = G.strided_out(rows, width, dtype, device="cpu")
    assert bool(g.untouched().all())
    g.check("fresh")
    g.view.copy_(torch.ones(rows, width).to(dtype))       # a kernel writing exactly its output
    g.check("exact")
    assert not bool(g.untouched().any())
    r0, c0 = g.origin
    for dr, dc in [(rows, 0), (-1, width - 1), (0, width), (2, -1), (rows + 255, 3)]:   # row below / above, column right / left
        h = G.strided_out(rows, width, dtype, device="cpu")
        h.buf[r0 + dr, c0 + dc] = 1
        with pytest.raises(AssertionError) as e:
            h.check("planted")
        assert "(row %d, column %d)" % (dr, dc) in str(e.value)


def test_output_pattern_is_a_signalling_nan_and_compared_by_bits():
    g = G.strided_out(2, 8, torch.float32, device="cpu")
    bits = g.buf.view(torch.int32)
    assert int(bits[0, 0]) == 0x7FA5A5A5 and bool(torch.isnan(g.buf).all())
    assert (0x7FA5A5A5 >> 22) & 1 == 0 and (0x7FA5 >> 6) & 1 == 0             # quiet bit clear
    g.buf[0, 0] = float("nan")                   # another NaN is still a write: a value comparison could not tell
    with pytest.raises(AssertionError):
        g.check("quiet NaN")


def test_flat_placement_and_guard():
    data = torch.arange(3 * 5 * 4, dtype=torch.float32).reshape(3, 5, 4)
    g = G.flat_in(data, device="cpu")
    assert g.view.is_contiguous() and torch.equal(g.view, data)
    assert (g.view.data_ptr() - g.buf.data_ptr()) % 256 == 0 and g.origin >= G.FLAT_GUARD
    assert bool(torch.isnan(g.buf[:g.origin]).all()) and bool(torch.isnan(g.buf[g.origin + data.numel():]).all())
    o = G.flat_out((3, 20), torch.int32, device="cpu")
    o.check("fresh")
    o.view.fill_(7)
    o.check("exact")
    o.buf[o.origin + 60] = 7                      # one element past the end
    with pytest.raises(AssertionError) as e:
        o.check("planted")
    assert "element 60 " in str(e.value)
    with pytest.raises(AssertionError):
        G.flat_in(torch.zeros(4, dtype=torch.int32), device="cpu")             # integer guards are chosen by the caller


def test_same_bits():
    a = torch.tensor([0.0, 1.0, float("nan")])
    assert G.same_bits(a, a.clone()) and not G.same_bits(a, torch.tensor([-0.0, 1.0, float("nan")]))
