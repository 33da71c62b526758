"""GPU parity: amx_combine_dev (combine_kernel) through rasr_amd.CombinedScorer against tests/posterior_reference.combine, which
tests/test_posterior.py holds against the reference's own results.  Everything is f32 in a fixed order, so every comparison is equality
of bits.

Shapes.  combine_kernel gives a workgroup of 256 lanes 1024 emissions of one frame: 1, 64, 65 emissions are below a workgroup's first
pass, 4099 takes five workgroups per frame with a ragged tail.  1, 2, 3 and 8 models (the most a handle takes); identity columns (read
straight) and permuted ones (read through the table) in every mix; every model's matrix has its own width and leading dimension with NaN
in the padding; the output is wider than n_emissions and pre-filled."""
import numpy as np
import pytest

from tests import posterior_reference as pr
from tests.test_posterior import refused, same

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
SCALES = (1.0, 0.1, 3.7, 0.5, 2.0, 1.0, 0.25, 1.5)


def case(n_models, n_emissions, T, seed):
    """model i: identity column for even i (width n_emissions), a gathered column into a matrix of its own width for odd i"""
    rng = np.random.Generator(np.random.PCG64(seed))
    table = np.zeros((n_emissions, n_models), np.int32)
    widths, mats = [], []
    for i in range(n_models):
        w = n_emissions if i % 2 == 0 else max(1, n_emissions // 2 + 3 * i)
        table[:, i] = np.arange(n_emissions) if i % 2 == 0 else rng.integers(0, w, n_emissions)
        m = rng.normal(50.0, 30.0, (T, w)).astype(np.float32)
        hit = rng.random(m.shape) < 0.03
        m[hit] = (1e4 + rng.normal(0.0, 50.0, m.shape)).astype(np.float32)[hit]
        widths.append(w)
        mats.append(m)
    return table, np.array(SCALES[:n_models], np.float32), widths, mats


@pytest.mark.parametrize("n_emissions", (1, 64, 65, 4099))
@pytest.mark.parametrize("n_models", (1, 2, 3, 8))
def test_combination_equals_the_restatement(ctx, n_models, n_emissions):
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    T = 67
    table, scales, widths, mats = case(n_models, n_emissions, T, 100 * n_models + n_emissions)
    want = pr.combine(table, scales, mats)
    if n_models >= 3 and n_emissions > 1:
        # from three models on the order of the terms matters to the bits (two terms commute): the test can fail
        assert not same(want, pr.combine(table[:, ::-1], scales[::-1], mats[::-1]))
    c = rasr_amd.CombinedScorer(ctx, widths, table, scales)
    straight = [bool(np.array_equal(table[:, i], np.arange(n_emissions))) for i in range(n_models)]
    assert c.identity_columns() == straight and (n_emissions == 1 or straight == [i % 2 == 0 for i in range(n_models)])
    lds = [w + 1 + i for i, w in enumerate(widths)]
    dev = []
    for m, ld in zip(mats, lds):
        wide = np.full((T, ld), np.nan, np.float32)
        wide[:, :m.shape[1]] = m
        dev.append(torch.from_numpy(wide).cuda())
    out = torch.full((T + 1, n_emissions + 2), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    c.combine(T, dev, lds, out, n_emissions + 2)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert same(got[:T, :n_emissions], want)
    assert np.all(got[:T, n_emissions:] == SENTINEL) and np.all(got[T] == SENTINEL)
    for part in (0, 1, 2):   # other batch sizes: the same bits, later rows untouched
        out2 = torch.full((T + 1, n_emissions + 2), float(SENTINEL), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        c.combine(part, dev, lds, out2, n_emissions + 2)
        torch.cuda.synchronize()
        g2 = out2.cpu().numpy()
        assert same(g2[:part, :n_emissions], want[:part]) and np.all(g2[part:] == SENTINEL)
    c.close()


def test_output_may_overlap_no_input(ctx):
    import rasr_amd
    import torch
    ctx.use_torch_stream()
    T, n = 5, 64
    c = rasr_amd.CombinedScorer(ctx, [n, n], np.stack([np.arange(n), np.arange(n)[::-1]], axis=1), [1.0, 2.0])
    a = torch.zeros((T, n), dtype=torch.float32, device="cuda")
    b = torch.ones((T, 2 * n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    refused(-1, "overlaps the scores of model 0", c.combine, T, [a, b], [n, 2 * n], a, n)
    refused(-1, "overlaps the scores of model 1", c.combine, T, [a, b], [n, 2 * n], b, 2 * n)
    refused(-1, "ld[1]", c.combine, T, [a, b], [n, n - 1], a, n)
    # the other column half of one matrix is no overlap (the views_alias rule)
    c.combine(T, [a, b], [n, 2 * n], b[:, n:], 2 * n)
    torch.cuda.synchronize()
    assert bool((b[:, :n] == 1).all()) and bool((b[:, n:] == 2).all())
    c.close()
