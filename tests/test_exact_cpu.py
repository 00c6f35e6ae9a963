"""CPU self-test of the integer-operand method (tests/_exact.py): an f32 matmul of the helper's operands passes
the bit-exact comparison in any K order, and each injected fault -- one product missing from one row, the last
K column dropped, a truncating bf16 store, a bias added twice -- fails it.  No GPU, no HIP kernel."""
import pytest
import torch

from tests._exact import (assert_bit_equal, assert_exact_domain, gemm_bound, int_tensor, is_bf16_tie, operand_hi)

SHAPES = [(37, 50, 200), (296, 200, 192)]


def _case(M, N, Kd):
    g = torch.Generator().manual_seed(M * 3 + N + Kd)
    h = operand_hi(Kd)
    a = int_tensor((M, Kd), -h, h, g)
    b = int_tensor((N, Kd), -h, h, g)
    bias = int_tensor((N,), -8, 8, g)
    assert_exact_domain(gemm_bound(a, b, bias, bias), a, b, bias)  # room for the doubled bias below
    ref = a.double() @ b.double().t() + bias.double()
    return g, a, b, bias, ref


def _truncate_bf16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)  # & 0xffff0000


@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_permuted_f32_matmul_is_bit_exact(M, N, Kd):
    g, a, b, bias, ref = _case(M, N, Kd)
    perm = torch.randperm(Kd, generator=g)
    c = a[:, perm] @ b[:, perm].t() + bias
    assert_bit_equal(c, ref, torch.float32, "f32")
    assert_bit_equal(c.to(torch.bfloat16), ref, torch.bfloat16, "bf16")


@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_one_missing_product_fails(M, N, Kd):
    g, a, b, bias, ref = _case(M, N, Kd)
    row, k = M // 2, Kd // 3
    if a[row, k] == 0:
        a[row, k] = 1.0  # the method's one blind spot is a zero product; the reference follows the operand
        ref = a.double() @ b.double().t() + bias.double()
    broken = a.clone()
    broken[row, k] = 0.0  # one product gone from every output of that row where b[n, k] != 0
    c = broken @ b.t() + bias
    with pytest.raises(AssertionError, match=rf"rows \[{row}, {row}\]"):
        assert_bit_equal(c, ref, torch.float32, "missing product")
    # a single output: zero the product of (row, col) alone
    col = int((b[:, k] != 0).nonzero()[0])
    c1 = a @ b.t() + bias
    c1[row, col] -= a[row, k] * b[col, k]
    with pytest.raises(AssertionError, match=rf"1 of {M * N} elements.*rows \[{row}, {row}\] x cols \[{col}, {col}\]"):
        assert_bit_equal(c1, ref, torch.float32, "missing product")


@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_dropped_last_k_column_fails(M, N, Kd):
    g, a, b, bias, ref = _case(M, N, Kd)
    c = a[:, :-1] @ b[:, :-1].t() + bias
    with pytest.raises(AssertionError, match="differ from the exact reference"):
        assert_bit_equal(c, ref, torch.float32, "k tail")


@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_truncating_bf16_store_fails(M, N, Kd):
    g, a, b, bias, ref = _case(M, N, Kd)
    c = a @ b.t() + bias
    assert_bit_equal(c.to(torch.bfloat16), ref, torch.bfloat16, "rne store")
    with pytest.raises(AssertionError, match="differ from the exact reference"):
        assert_bit_equal(_truncate_bf16(c), ref, torch.bfloat16, "truncating store")


@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_double_bias_fails(M, N, Kd):
    g, a, b, bias, ref = _case(M, N, Kd)
    c = a @ b.t() + bias + bias
    with pytest.raises(AssertionError, match="differ from the exact reference"):
        assert_bit_equal(c, ref, torch.float32, "double bias")


def test_bf16_case_without_rounding_is_rejected():
    """A bf16 comparison whose reference never needs rounding would not test the store: rejected as a broken
    case, as is one without an exact tie."""
    ref = torch.arange(-200, 200, dtype=torch.float64).view(20, 20)
    with pytest.raises(AssertionError, match="needs bf16 rounding"):
        assert_bit_equal(ref.to(torch.bfloat16), ref, torch.bfloat16, "small")
    ref = torch.full((4, 4), 1025.0, dtype=torch.float64)  # rounds (to 1024) but is no tie
    with pytest.raises(AssertionError, match="exact bf16 tie"):
        assert_bit_equal(ref.to(torch.bfloat16), ref, torch.bfloat16, "no tie")
    t = torch.tensor([255.0, 257.0, 258.0, 514.0, 516.0, 1026.0, -301.0], dtype=torch.float64)
    assert is_bf16_tie(t).tolist() == [False, True, False, True, False, False, True]


def test_exact_domain_rejects():
    g = torch.Generator().manual_seed(0)
    a = int_tensor((8, 250), 200, 256, g)
    b = int_tensor((8, 250), 200, 256, g)
    assert gemm_bound(a, b) < 2 ** 24
    assert_exact_domain(gemm_bound(a, b), a, b)
    big = torch.cat([a, a], 1)
    assert gemm_bound(big, torch.cat([b, b], 1)) >= 2 ** 24  # 500 products of about 2^16
    with pytest.raises(AssertionError, match="2\\^24"):
        assert_exact_domain(gemm_bound(big, torch.cat([b, b], 1)), big)
    with pytest.raises(AssertionError, match="non-integer"):
        assert_exact_domain(10.0, torch.tensor([1.0, 2.5]))
    with pytest.raises(AssertionError, match="exceeds"):
        assert_exact_domain(10.0, torch.tensor([1.0, 257.0]))
