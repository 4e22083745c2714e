"""The attention edge cases of tests/test_gpu_model_edges.py, checked without a
GPU: oracle/attn_edges.py emulates the arithmetic the HIP kernels are meant to
perform (fp32 logits, 64-key blocks with the lazy +8 rescale, bf16 P, fp32
accumulation; backward from the log-sum-exp with bf16 dS and P).  These tests
prove that each input kind still does what its name says (the rescale path of
k_attention runs, p reaches the 2^8 regime) and that the intended arithmetic
sits inside every bound the GPU test applies to the kernels, so a failure
there is the kernel's."""
import pytest

from oracle import attn_edges as E


@pytest.fixture(scope="module")
def table():
    out = {}
    for r, s, heads in E.SHAPES:
        for kind in E.KINDS:
            for mask in E.MASKS:
                c = E.case(kind, mask, r, s, heads)
                em = E.emulate(c.qkv, c.d_out, c.ids, c.kp, r, s, heads)
                out[kind, mask, r, s, heads] = (c, em)
    return out


def test_inputs_are_bf16_exact_and_masks_have_their_shape(table):
    for (kind, mask, r, s, heads), (c, _) in table.items():
        assert E.bf(c.qkv).equal(c.qkv) and E.bf(c.d_out).equal(c.d_out)
        if mask == "nopad":
            assert not c.kp.any() and (s < 3 or c.ids[0].unique().numel() == 3)
        if mask == "allpad":
            assert c.kp[0].all() and not c.kp[1, :s // 2].any() and c.kp[1, s // 2:].all()
        if mask == "scatter" and s >= 200:
            pad_ids = c.ids[c.kp].unique()
            assert pad_ids.numel() == 4   # pad keys of several images: the +1 bias hits queries of every id
            blocks = [c.kp[0, k0:k0 + 64].any().item() for k0 in range(0, s, 64)]
            assert any(blocks)


def test_each_kind_drives_the_path_it_is_named_for(table):
    print("\nkind mask shape: rescales after block 0, p max")
    for (kind, mask, r, s, heads), (_, em) in table.items():
        print(f"  {kind:5s} {mask:7s} {(r, s, heads)}: {em.rescales:5d} {em.pmax:.4g}")
        if kind in ("plain", "down"):
            assert em.rescales == 0
        if kind == "fast" and s > 64:
            assert em.rescales >= r * heads * (s - 64) // 64   # every query, at every later block
        if kind in ("fast", "slow", "saw") and s >= 257:
            assert em.rescales > 0
        if kind == "slow" and s >= 257:
            assert em.pmax > 128
        assert em.pmax <= 2.0 ** 8 * 1.0001   # the lazy rescale's promise


def test_the_intended_arithmetic_meets_every_bound(table):
    worst = dict(fwd=0.0, lse=0.0, grad=0.0, rows=0.0)
    for (kind, mask, r, s, heads), (c, em) in table.items():
        fwd, lse = E.forward_ratio(em.out, c.ref), E.lse_error(em.lse, c.ref)
        gr = E.grad_ratios(em.dqkv, c.ref, 64 * heads)
        rows = gr.pop("dq rows")
        worst = dict(fwd=max(worst["fwd"], fwd), lse=max(worst["lse"], lse), grad=max(worst["grad"], *gr.values()),
                     rows=max(worst["rows"], rows))
        assert fwd <= 1.0, (kind, mask, r, s, heads, fwd)
        assert lse <= 1e-4, (kind, mask, r, s, heads, lse)
        assert max(gr.values()) <= 1.0, (kind, mask, r, s, heads, gr)
        assert rows <= 1.0, (kind, mask, r, s, heads, rows)
    print(f"\nworst forward error / bound {worst['fwd']:.3f}, lse error {worst['lse']:.3g}, "
          f"gradient deviation / allowance {worst['grad']:.3f}, per dq row {worst['rows']:.3f}")
