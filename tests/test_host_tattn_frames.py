"""CPU: temporal attention at 64 / 96 / 128 frames (csrc/sdc_tattn_frames.hip) without a GPU.
  * the references of tests/test_gpu_tattn_frames.py are sound: the same formula in fp32 torch meets that file's gates against
    fp64 with a factor of four to spare on the plain and far-peak inputs, and the max(gate, 4 e_fp32) rule of the scale-4 case
    never lifts a gate past four times the file gate;
  * sdc_attn_route, the one predicate sdc_attn and sdc_attn_bwd dispatch through: the frames domain, today's routes next to it,
    the refusals and their wording, independence of `outer`;
  * sdc_attn_bwd_bytes keeps its values outside the frames domain;
  * the fixture tests/golden/smoke_unet_f64.npz (the real reference at 64 frames, tools/make_smoke_frames_fixture.py) is what
    oracle.nets.unet_smoke computes: eps bit for bit, gradients to 1e-5."""
import pytest
import torch

import tattn_frames_ref as R
from oracle import nets as onets
from oracle.detweights import det_params, det_tensor
from safediffcon_amd import _lib

SDC_EINVAL = -1


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_fp32_formula_meets_the_gates_with_room(shape, scale):
    e = R.err32("plain", *shape, scale)
    print(f"[measured] fp32 torch vs fp64, {shape} x {scale:g}: out {e[0]:.2e} dqkv {e[1]:.2e} dbias {e[2]:.2e}")
    assert 4 * e[0] <= R.GATE_OUT and 4 * e[1] <= R.GATE_GRAD and 4 * e[2] <= R.GATE_GRAD


@pytest.mark.parametrize("shape", R.FAR)
def test_fp32_formula_meets_the_gates_on_far_peaks(shape):
    qkv, bias, _ = R.far_peak(*shape)
    F_ = shape[0]
    # the bump does what it says: every row's largest bias sits F/2 keys from the diagonal, in another 32-key block
    i = torch.arange(F_)
    assert bool((bias.argmax(-1) == (i + F_ // 2) % F_).all()) and bool((((i + F_ // 2) % F_) // 32 != i // 32).all())
    e = R.err32("far", *shape)
    print(f"[measured] fp32 torch vs fp64, far peak {shape}: out {e[0]:.2e} dqkv {e[1]:.2e} dbias {e[2]:.2e}")
    assert 4 * e[0] <= R.GATE_OUT and 4 * e[1] <= R.GATE_GRAD and 4 * e[2] <= R.GATE_GRAD


@pytest.mark.parametrize("shape", R.PEAKED)
def test_scale_4_rule_stays_within_four_file_gates(shape):
    e = R.err32("plain", *shape, 4.0)
    print(f"[measured] fp32 torch vs fp64, {shape} x 4: out {e[0]:.2e} dqkv {e[1]:.2e} dbias {e[2]:.2e}")
    assert R.gate(R.GATE_OUT, e[0]) <= 4 * R.GATE_OUT
    assert R.gate(R.GATE_GRAD, e[1]) <= 4 * R.GATE_GRAD and R.gate(R.GATE_GRAD, e[2]) <= 4 * R.GATE_GRAD


# ------------------------------------------------------------------ routing
def _route(inner, ntok, q_si, q_st, o_si, o_st, rot=1, bias=1, dbias=0, backward=0):
    return _lib.get_lib().sdc_attn_route(inner, ntok, q_si, q_st, o_si, o_st, rot, bias, dbias, backward)


def _strided(inner, ntok, **kw):
    """frame-strided dense tensors: pixels contiguous, frames `inner` apart"""
    return _route(inner, ntok, 1, inner, 1, inner, **kw)


def _contig(inner, ntok, **kw):
    return _route(inner, ntok, ntok, 1, ntok, 1, rot=0, bias=0, **kw)


@pytest.mark.parametrize("ntok", [64, 96, 128])
@pytest.mark.parametrize("inner", [3, 4, 15, 64, 4096])
def test_frames_domain_routes_to_the_frames_kernels(ntok, inner):
    for rot in (0, 1):
        for bias in (0, 1):
            assert _strided(inner, ntok, rot=rot, bias=bias) == 4
            assert _strided(inner, ntok, rot=rot, bias=bias, backward=1) == 4
            assert _strided(inner, ntok, rot=rot, bias=bias, dbias=1, backward=1) == 4


def test_todays_routes_are_unchanged():
    assert _strided(64, 32) == 1 and _strided(64, 32, backward=1) == 1 and _strided(64, 32, dbias=1, backward=1) == 1
    assert _strided(3, 32) == 0 and _strided(3, 32, backward=1) == 0            # inner % 8 != 0: the generic kernels
    for ntok in (8, 48, 160):
        assert _strided(64, ntok) == 0 and _strided(64, ntok, backward=1) == 0
    assert _strided(64, 8, dbias=1, backward=1) == 0
    assert _contig(4, 256) == 2 and _contig(4, 256, backward=1) == 0
    assert _contig(4, 257) == 3 and _contig(4, 257, backward=1) == 3
    assert _contig(4, 64) == 0 and _contig(4, 64, backward=1) == 0               # 64 contiguous tokens are not frames
    # pixels two apart at 64 frames: outside the frames domain
    assert _route(64, 64, 2, 128, 2, 128) == 0 and _route(64, 64, 2, 128, 2, 128, backward=1) == 0
    assert _route(64, 64, 1, 64, 2, 128) == 0
    # the 32-bit lane-offset rule: frame stride x ntok x 4 bytes < 2^32 for both tensors
    assert _route(64, 64, 1, (1 << 24) - 1, 1, 64) == 4 and _route(64, 64, 1, 1 << 24, 1, 64) == 0
    assert _route(64, 128, 1, 64, 1, 1 << 23) == 0 and _route(64, 128, 1, 64, 1, 1 << 23, backward=1) == 0


def test_refused_bias_gradients_name_the_new_limit():
    for rc in (_strided(64, 160, dbias=1, backward=1), _route(64, 64, 2, 128, 2, 128, dbias=1, backward=1)):
        assert rc == SDC_EINVAL
        msg = _lib.last_error()
        assert "ntok <= 32" in msg and "64, 96 or 128 frames with contiguous pixels" in msg, msg
    assert _contig(4, 300, dbias=1, backward=1) == SDC_EINVAL and "more than 256 tokens" in _lib.last_error()
    assert _route(4, 300, 1, 4, 1, 4) == SDC_EINVAL and "more than 256 tokens" in _lib.last_error()


def test_route_has_no_outer_argument():
    """the result cannot change with `outer`: the predicate does not take it (nor heads, nor a pointer)"""
    _, argtypes = _lib.SIGNATURES["sdc_attn_route"]
    assert len(argtypes) == 10
    for outer in (1, 2, 64):
        assert _strided(16, 64) == 4                    # whatever the batch


# ------------------------------------------------------------------ workspace
def test_bwd_bytes_outside_the_frames_domain_are_todays():
    lib = _lib.get_lib()
    assert int(lib.sdc_attn_bwd_bytes(2, 64, 4, 8)) == 1048576            # 1024 slots x 4 heads x 8 x 8 floats
    assert int(lib.sdc_attn_bwd_bytes(2, 64, 4, 32)) == 16777216
    assert int(lib.sdc_attn_bwd_bytes(2, 64, 4, 320)) == 1310720          # the streaming kernels' row statistics
    for ntok in (64, 96, 128):                                            # fewer slots, the same for every batch
        b = int(lib.sdc_attn_bwd_bytes(2, 64, 4, ntok))
        assert b == int(lib.sdc_attn_bwd_bytes(7, 4096, 4, ntok)) and b % (16 * ntok * ntok) == 0
        assert b < 1024 * 4 * ntok * ntok * 4


# ------------------------------------------------------------------ the fixture
def test_fixture_is_what_the_oracle_computes(golden):
    g = golden("smoke_unet_f64")
    dim, Fr, S = int(g.scalar("dim")), int(g.scalar("frames")), int(g.scalar("image_size"))
    # (the rotary frequencies are not learnable in the reference: their stored gradient is zero)
    P = {k: v.requires_grad_(v.is_floating_point() and not k.endswith("rotary_emb.freqs"))
         for k, v in det_params(g.spec(), int(g.scalar("weight_seed"))).items()}
    x = det_tensor((1, Fr, 7, S, S), int(g.scalar("x_seed")))
    eps = onets.unet_smoke(P, x, g["t"], dim=dim, dim_mults=(1, 2, 4))
    assert torch.equal(eps.detach(), g["eps"])
    target = det_tensor((1, Fr, 7, S, S), int(g.scalar("target_seed")))
    loss = (g["w"] * ((eps - target) ** 2).flatten(1).mean(1)).mean()
    loss.backward()
    assert abs(loss.item() - g.scalar("loss")) <= 1e-6 * abs(g.scalar("loss"))
    keys = [str(k) for k in g["grad_keys"]]
    assert "time_rel_pos_bias.relative_attention_bias.weight" in keys
    seed, worst, whole = int(g.scalar("dot_seed")), 0.0, 0
    gmax = float(g.z["grad_norms"].max())
    for i, k in enumerate(keys):
        gr = (P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])).double()
        n_ref = float(g.z["grad_norms"][i])
        if n_ref < 1e-4 * gmax:             # zero in exact arithmetic (a conv bias in front of a GroupNorm): rounding noise
            assert gr.norm().item() < 2e-4 * gmax, k
            continue
        proj = det_tensor(tuple(gr.shape), seed + i).double()
        e = max(abs(gr.norm().item() - n_ref) / n_ref, abs((gr * proj).sum().item() - float(g.z["grad_dots"][i])) / (n_ref * proj.norm().item()))
        if "grad:" + k in g.keys():
            full = g["grad:" + k].double()
            e = max(e, ((gr - full).norm() / full.norm()).item())
            whole += 1
        worst = max(worst, e)
        assert e < 1e-5, (k, e)
    print(f"[measured] oracle vs the reference at {Fr} frames: eps equal bits, {len(keys)} gradients ({whole} stored whole), worst relative L2 {worst:.2e}")
