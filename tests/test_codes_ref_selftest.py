"""CPU-only checks of the float64 reference of decode-from-codes (tests/codes_ref.py), on the inputs tests/test_gpu_codes.py uses: it is the
oracle's own forward when the codes are the utterance's own, each code depends on its own input alone (eval mode), and every indexing
mistake a decode-from-codes can make lands at least 100 x the GPU tests' bar (1e-4) away from the right answer."""
import pytest
import torch

import codes_ref as R
from oracle import ref_model

HP = R.HP
B, T = 3, 24
FAR = 1e-2                         # 100 x the GPU tests' f32 bar


@pytest.fixture(scope='module')
def case():
    mel, onehot, emb = R.inputs(R.SEED_IN, B, T)
    x_f0 = torch.cat((mel, onehot), -1)
    x_org = R.inputs(R.SEED_IN + 1, B, T)[0]
    P = R.p64('G3')
    codes = R.encode_g3(P, HP, x_f0, x_org)
    return P, x_f0, x_org, emb, codes, R.decode_g3(P, HP, *codes, emb)


def test_decode_of_encode_is_the_oracle_forward(case):
    P, x_f0, x_org, emb, codes, out = case
    with torch.no_grad():
        ref = ref_model.generator_3(P, HP, x_f0.double(), x_org.double(), emb.double())
    assert torch.equal(out, ref)
    P6 = R.p64('G6')
    mel, onehot, _ = R.inputs(R.SEED_IN, B, T)
    with torch.no_grad():
        ref6 = ref_model.generator_6(P6, HP, mel.double(), onehot.double())
    assert torch.equal(R.decode_g6(P6, HP, *R.encode_g6(P6, HP, mel, onehot)), ref6)


def test_code_shapes_and_layout(case):
    _, _, _, _, (cx, c2, cf), out = case
    assert cx.shape == (B, T // HP.freq, 2 * HP.dim_neck) and c2.shape == (B, T // HP.freq_2, 2 * HP.dim_neck_2)
    assert cf.shape == (B, T // HP.freq_3, 2 * HP.dim_neck_3) and out.shape == (B, T, HP.dim_freq)
    o = torch.arange(2 * 8 * 6, dtype=torch.float64).reshape(2, 8, 6)
    c = ref_model.codes_from(o, 3, 4)          # forward half at the LAST frame of each block, backward half at the FIRST
    assert torch.equal(c[:, :, :3], o[:, [3, 7], :3]) and torch.equal(c[:, :, 3:], o[:, [0, 4], 3:])


def test_each_code_depends_on_its_own_input_alone(case):
    """eval mode: content <- mel columns, pitch <- one-hot columns, rhythm <- x_org; the dependence on the others is exactly zero"""
    P, x_f0, x_org, _, (cx, c2, cf), _ = case
    other = R.inputs(99, B, T)
    mel, onehot = x_f0[..., :HP.dim_freq], x_f0[..., HP.dim_freq:]
    ax, a2, af = R.encode_g3(P, HP, torch.cat((mel, other[1]), -1), other[0])            # pitch input and x_org replaced
    assert torch.equal(ax, cx) and not torch.equal(af, cf) and not torch.equal(a2, c2)
    bx, b2, bf = R.encode_g3(P, HP, torch.cat((other[0], onehot), -1), x_org)            # mel columns replaced
    assert torch.equal(bf, cf) and torch.equal(b2, c2) and not torch.equal(bx, cx)


def test_every_wrong_variant_is_far_from_the_right_answer(case):
    P, _, _, emb, codes, out = case
    variants = R.wrong_variants(*codes, emb)
    assert len(variants) == 3 * 3 + 2
    for name, args in variants.items():
        r = R.rel(R.decode_g3(P, HP, *args), out)
        print(f'[wrong variant {name}] rel {r:.3e}')
        assert r >= FAR, (name, r)


def test_a_padded_row_is_far_from_the_row_alone(case):
    """what a ragged decode that ignored the lengths would give: row 1 decoded over 24 frames against the row decoded alone at 8"""
    P, x_f0, x_org, emb, codes, out = case
    n = 8
    alone = R.decode_g3(P, HP, *R.encode_g3(P, HP, x_f0[1:2, :n], x_org[1:2, :n]), emb[1:2])
    r = R.rel(out[1:2, :n], alone)
    print(f'[padded row vs alone] rel {r:.3e}')
    assert r >= FAR
