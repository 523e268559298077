"""Real-time chunking by inpainting, host side: `chunking.shift_chunk` / `RealTimeChunker`, the argument checks of
`sample_actions(inpaint=...)`, the time grid, and the inpainting loop restated on the oracle's pieces (tests/inpaint_reference.py)."""
import fractions
import inspect

import numpy as np
import pytest
import torch

from oracle import lap_oracle as O
from tests.common import debug_model_cfg, make_inputs, oracle_cfg
from tests.inpaint_reference import fma_f32, oracle_sample_inpaint, replay_steps


def _prev(S=6, ad=3):
    return np.arange(S * ad, dtype=np.float32).reshape(S, ad) + 1.0


@pytest.mark.parametrize("executed,freeze", [(0, 0), (0, 6), (0, 3), (2, 0), (2, 4), (2, 1), (6, 0), (5, 1)])
def test_shift_chunk(executed, freeze):
    from lap_amd.chunking import shift_chunk

    prev = _prev()
    S = prev.shape[0]
    known, mask = shift_chunk(prev, executed, freeze)
    assert known.dtype == np.float32 and known.shape == prev.shape and mask.dtype == np.uint8 and mask.shape == (S,)
    for h in range(S):
        want = prev[h + executed] if h + executed < S else np.zeros(prev.shape[1], np.float32)
        assert np.array_equal(known[h], want), h
        assert mask[h] == (1 if h < freeze else 0), h
    assert np.array_equal(prev, _prev())      # the previous chunk is left alone
    kb, mb = shift_chunk(np.stack([prev, 2 * prev]), executed, freeze)      # batched
    assert np.array_equal(kb[0], known) and np.array_equal(kb[1], 2 * known) and np.array_equal(mb, np.stack([mask, mask]))


@pytest.mark.parametrize("executed,freeze", [(-1, 0), (7, 0), (0, -1), (0, 7), (2, 5), (6, 1), (1.0, 0), (0, True)])
def test_shift_chunk_rejects_out_of_range(executed, freeze):
    from lap_amd.chunking import shift_chunk

    with pytest.raises(ValueError):
        shift_chunk(_prev(), executed, freeze)
    with pytest.raises(ValueError):
        shift_chunk(np.zeros(5, np.float32), 0, 0)


def test_real_time_chunker():
    from lap_amd.chunking import RealTimeChunker, shift_chunk

    c = RealTimeChunker()
    assert c.next(2, 3) is None and c.next(99, 99) is None      # no previous chunk: nothing to shift, nothing to check
    buf = _prev()
    c.update(buf)
    buf[:] = -1.0       # the chunker keeps a copy
    for executed, freeze in ((0, 0), (0, 6), (2, 4), (2, 0)):
        known, mask = c.next(executed, freeze)
        wk, wm = shift_chunk(_prev(), executed, freeze)
        assert np.array_equal(known, wk) and np.array_equal(mask, wm)
    with pytest.raises(ValueError):
        c.next(2, 5)
    c.update(2 * _prev())
    assert np.array_equal(c.next(1, 1)[0], shift_chunk(2 * _prev(), 1, 1)[0])
    c.reset()
    assert c.next(0, 0) is None
    with pytest.raises(ValueError):
        c.update(np.zeros(4))


def test_inpaint_times():
    from lap_amd.flow_sample import inpaint_times

    for n in (1, 3, 10):
        ts = inpaint_times(n)
        assert len(ts) == n and ts[-1] == (0.0, 1.0)
        for k, (tp, omtp) in enumerate(ts):
            assert tp == (n - 1 - k) / n and omtp == 1.0 - tp and isinstance(tp, float)
    assert inpaint_times(10)[0] == (0.9, 1.0 - 0.9)


def test_argument_checks():
    from lap_amd.flow_sample import check_inpaint

    B, S, ad = 2, 5, 3
    known, mask = torch.randn(B, S, ad), torch.zeros(B, S)
    mask[0, :2] = 1
    k, m = check_inpaint((known, mask), B, S, ad, "cpu")
    assert k.dtype == torch.float32 and m.dtype == torch.uint8 and torch.equal(k, known) and torch.equal(m.float(), mask)
    k, m = check_inpaint((known.numpy().astype(np.float64), mask.bool().numpy()), B, S, ad, "cpu")      # arrays, bool masks
    assert k.dtype == torch.float32 and torch.equal(m.float(), mask)
    bad = [
        (known[:1], mask[:1]),                    # batch mismatch
        (known[:, :4], mask),                     # wrong horizon
        (known[..., :2], mask),                   # wrong action_dim (un-padded)
        (known, mask[:, :4]),
        (known, mask[..., None].expand(B, S, ad)),      # one flag per ROW
        (known[0], mask[0]),
        (torch.where(mask.bool()[..., None], torch.nan, known), mask),
        (known.clone().index_fill_(1, torch.tensor([4]), float("inf")), mask),
        (known, mask * 2),
        (known, mask - 1),
        (known, mask + 0.5),
        (known,),
        known,
    ]
    for i, arg in enumerate(bad):
        with pytest.raises(ValueError):
            check_inpaint(arg, B, S, ad, "cpu")
            pytest.fail(f"case {i} accepted")


def test_public_signatures_default_to_no_inpainting():
    from lap_amd import flow_sample
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedSampler

    for fn in (LAP.sample_actions, flow_sample.sample_actions):
        assert inspect.signature(fn).parameters["inpaint"].default is None
    assert "NOT in the reference" in (inspect.getdoc(LAP.sample_actions) or "")
    assert inspect.signature(GraphedSampler.__init__).parameters["inpaint"].default is False
    assert "not in the reference" in (inspect.getdoc(GraphedSampler) or "").lower()


def test_fma_restatement_rounds_once():
    """`fma_f32` against exact rational arithmetic rounded once to f32, on random operands and on sums built to fall next to a
    rounding boundary of the float64 sum (where rounding twice goes wrong)."""
    def exact(a, b, c):
        q = fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))
        lo = np.float32(float(q))           # within one spacing of the answer
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda f: (abs(fractions.Fraction(float(f)) - q), int(np.float32(f).view(np.int32)) & 1))
        return float(best)

    g = torch.Generator().manual_seed(0)
    a = torch.tensor(-1.0 / 3.0, dtype=torch.float32).item()
    b, c = torch.randn(400, generator=g), torch.randn(400, generator=g)
    # halfway cases of the final rounding with a product bit far below: c = an odd multiple of half an f32 spacing is not an f32,
    # so build them from the product side: b tiny, c a number whose sum with a * b sits within 2^-60 of a midpoint
    tiny = torch.tensor([2.0 ** -40, -2.0 ** -40, 2.0 ** -45, -2.0 ** -33], dtype=torch.float32)
    mid = torch.tensor([1.0 + 2.0 ** -23, 1.0 + 3 * 2.0 ** -23, -1.0 - 2.0 ** -23, 2.0 + 2.0 ** -22], dtype=torch.float32)
    b, c = torch.cat([b, tiny, tiny]), torch.cat([c, mid, mid.flip(0)])
    got = fma_f32(a, b, c)
    for i in range(b.numel()):
        assert got[i].item() == exact(a, b[i].item(), c[i].item()), i


def test_oracle_restatement_of_the_inpainting_loop():
    """Frozen rows of the result equal `known` exactly; an all-zero mask gives `O.sample_actions`; the frozen head changes the free
    rows; and the host replay of the steps reproduces the restatement's frozen rows at every step count."""
    cfg = debug_model_cfg()
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=11)
    obs, _, noise, _ = make_inputs(cfg, B=2, ragged=True)
    so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
    S = cfg.action_horizon
    g = torch.Generator().manual_seed(3)
    known = torch.randn(noise.shape, generator=g)
    plain = O.sample_actions(P, oc, so, noise, num_steps=3)
    zero = torch.zeros(2, S, dtype=torch.uint8)
    assert torch.equal(oracle_sample_inpaint(P, oc, so, noise, known, zero, num_steps=3), plain)
    mask = zero.clone()
    mask[0, :S // 2] = 1
    mask[1, S - 1] = 1
    col = {}
    out = oracle_sample_inpaint(P, oc, so, noise, known, mask, num_steps=3, collect=col)
    fr = mask.bool()
    assert torch.equal(out[fr], known[fr])
    assert not torch.equal(out[~fr], plain[~fr]) and bool(torch.isfinite(out).all())
    assert sorted(col) == ["v_t/0", "v_t/1", "v_t/2"]
    rep = replay_steps(noise, known, mask, [col[f"v_t/{k}"] for k in range(3)], -1.0 / 3)
    assert torch.equal(rep[fr], known[fr])
    assert torch.allclose(rep, out, rtol=0, atol=1e-5)      # (the oracle's free update rounds the product: not the same bits)
