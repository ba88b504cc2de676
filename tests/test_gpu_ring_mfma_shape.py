"""The narrow fp32-output ring tiles and the MFMA shape they run (csrc/gemm_bf16.hip, S16), forced through the unit C ABI in both
operand formats: the 8-wave tiles on v_mfma_f32_16x16x32 -- 49 (128 x 128 on two K-groups of 64 x 64 waves), 15 and 44 (128 x 128, eight
waves of 32 x 64, 3- and 4-stage ring) -- and the 4-wave tile 16 (128 x 64), which measured slower on that shape and stays on 32 x 32 x 16:
the same checks hold it to the same results.

What the MFMA shape changes is the fragment a lane reads, the (row, column) a lane's accumulator registers stand for, and the row
blocks the two K-groups exchange; so the tests are an exact selection test (any permutation of rows, columns or k shows), the tile
edges against float64 with a bound that holds for every summation order, and the LayerNorm-fold producer behind the same accumulators."""
import pytest
import torch

from test_gpu_kernels import _ln_fold_producer
from util import FORMATS, guarded

pytestmark = pytest.mark.gpu

# tile id -> columns of one tile.  The C ABI takes N in multiples of 128 (sat_launch_gemm), so tile 16 never runs a single 64-column
# tile: its smallest case is two of them.
TILES = {49: 128, 15: 128, 44: 128, 16: 64}


def _lib():
    from stable_audio_tools import _hip
    return _hip, _hip.lib()


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _gemm(dev, fmt, a, w, bias, c0, tile):
    """C = a w^T (+ bias) (+ c0) on the forced tile, into a guarded buffer; returns the fp32 result on the host."""
    _hip, lib = _lib()
    m, k = a.shape
    n = w.shape[0]
    ad, wd = a.to(dev), w.to(dev)
    bd = bias.to(dev) if bias is not None else None
    cg = guarded((m, n), torch.float32, dev, init=c0, name=f"c of tile {tile}")
    _hip.check(fmt.fn(lib, "sat_gemm_bf16_f32")(_hip.ptr(ad), _hip.ptr(wd), _hip.ptr(bd) if bd is not None else None, _hip.ptr(cg.t), m, n, k,
                                                 1 if c0 is not None else 0, tile, _hip.stream()))
    # the rows from M on (the NaN guard: 256 rows on each side) are untouched, every row below M is written
    cg.check().assert_written()
    return cg.t.cpu()


def _one_hot(rows, k):
    x = torch.zeros(rows, k)
    idx = (7 * torch.arange(rows) + 3) % k          # 7 is a unit mod 256: distinct k for distinct rows
    x[torch.arange(rows), idx] = 1.0
    return x, idx


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("one_hot", ["a", "w"])
@pytest.mark.parametrize("tile", sorted(TILES))
def test_fragment_and_accumulator_mapping_exact(dev, tile, one_hot, fmt):
    """A one-hot operand turns the product into a selection of the other operand's values: the output is exact, and a permuted row,
    column or k index, or a swapped row block of the K-group exchange, moves a value to where torch.equal sees it."""
    m, n, k = 128, 128, 256
    if one_hot == "a":
        a, idx = _one_hot(m, k)
        w = _rand((n, k), 11)
        a, w = a.to(fmt.dtype), w.to(fmt.dtype)
        want = w.float()[:, idx].T          # c[m, n] = w[n, idx[m]]
    else:
        w, idx = _one_hot(n, k)
        a = _rand((m, k), 12)
        a, w = a.to(fmt.dtype), w.to(fmt.dtype)
        want = a.float()[:, idx]            # c[m, n] = a[m, idx[n]]
    got = _gemm(dev, fmt, a, w, None, None, tile)
    bad = (got != want).nonzero()
    assert torch.equal(got, want), f"tile {tile}, one-hot {one_hot}: {bad.shape[0]} elements differ, the first at {tuple(bad[0].tolist())}"


# One float64 reference per (format, K, columns) at the tallest M, shared by the M cases (rows are independent: the first M rows of the
# operands give the first M rows of the product); never modified.
_REF = {}


def _edge_case(fmt, k, n):
    key = (fmt.name, k, n)
    if key not in _REF:
        m = 161
        a = _rand((m, k), 21).to(fmt.dtype)
        w = (_rand((n, k), 22) * 0.05 + torch.linspace(-0.02, 0.03, n)[:, None]).to(fmt.dtype)
        bias = _rand((n,), 23)
        c0 = _rand((m, n), 24)
        prod = a.double() @ w.double().T
        mag = a.double().abs() @ w.double().abs().T          # sum |a w| of the row and column
        _REF[key] = (a, w, bias, c0, prod, mag)
    return _REF[key]


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("k", [256, 384, 1536])
@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("m", [1, 127, 130, 161])
@pytest.mark.parametrize("tile", sorted(TILES))
def test_edges_against_float64(dev, tile, m, n, k, fmt):
    """M = 130: a 2-row tail tile whose upper waves have no valid rows; M = 161: a wave tile where K-group 0's 32 finishing rows are
    valid and group 1's start beyond M.  K = 256 is the shortest reduction the two-group ring takes, 384 an odd slice count (the drain
    path).  N = 128 and 256 are one and two column tiles of the 128-column tiles, two and four of tile 16.  With and without accumulation and bias.

    Bound per element: (K + 4) 2^-24 sum |a w|.  The products of two 16-bit operands are exact in fp32, so K - 1 additions in ANY order
    stay within (K - 1) 2^-24 sum |a w| to first order; the bias and residual additions round twice more, by at most
    2^-24 (2 sum|a w| + 2 |bias| + |c0|), which the remaining 5 units cover as long as 2 |bias| + |c0| <= 3 sum |a w| (asserted on the
    inputs).  A dropped or doubled product is an error of |a w| ~ sum |a w| / K, thousands of times the bound."""
    a, w, bias, c0, prod, mag = _edge_case(fmt, k, n)
    a, c0, prod, mag = a[:m], c0[:m], prod[:m], mag[:m]
    assert bool((2 * bias.double().abs() + c0.double().abs() <= 3 * mag).all()), "inputs: the epilogue's roundings must fit the bound"
    bound = (k + 4) * 2.0 ** -24 * mag
    for accumulate in (False, True):
        for with_bias in (False, True):
            got = _gemm(dev, fmt, a, w, bias if with_bias else None, c0 if accumulate else None, tile).double()
            want = prod + (bias.double() if with_bias else 0.0) + (c0.double() if accumulate else 0.0)
            excess = (got - want).abs() / bound
            worst = excess.argmax()
            r, c = divmod(int(worst), n)
            print(f"tile {tile} {fmt} {m}x{n}x{k} accumulate={accumulate} bias={with_bias}: worst |error| / bound {float(excess.max()):.3f} at ({r}, {c})")
            assert float(excess.max()) <= 1.0, (f"tile {tile} {m}x{n}x{k} accumulate={accumulate} bias={with_bias}: element ({r}, {c}) is "
                                                f"{float(excess.max()):.2f} x the summation-order bound off the float64 product")


@pytest.mark.parametrize("fmt", FORMATS, ids=repr)
@pytest.mark.parametrize("n", [128, 384])
@pytest.mark.parametrize("tile", sorted(TILES))
def test_ln_fold_producer_behind_both_accumulator_layouts(dev, tile, n, fmt):
    """The 16-bit image is the rounding of the fp32 row just written and (sum, sum of squares) per 64 columns are those of the rounded
    values: the checks of test_gpu_kernels._ln_fold_producer, at a 2-row tail tile of the forced tiles.  (The C ABI takes N in multiples
    of 128, so the odd count of column tiles is 384 = three 128-column tiles, not 192.)"""
    _ln_fold_producer(dev, 130, n, 256, tile, seed=60, fmt=fmt)
