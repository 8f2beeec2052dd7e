"""The recurrent regressors without a GPU (soft-grip_amd/lstm.py): the layer's torch implementation against torch.nn.LSTM and the NumPy
restatement (tests/np_lstm.py), direction semantics, initialisers, dropout, parameter counts, the nets' shapes and training step, the
two entry points' argument checks and the kernels' kept assembly.  TensorFlow is not available to produce golden outputs."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import np_lstm as npl
from softgrip_amd import convnet as cn
from softgrip_amd import lstm as L

TOL = 1e-13       # absolute; two CPU summation orders differ by 4e-16 on h at (100, 25, 256, 128)


def _nn_lstm(layers, D, H):
    """torch.nn.LSTM (double) carrying the layers' weights: one KerasLSTM, or (fwd, bwd) for a bidirectional one"""
    ref = torch.nn.LSTM(D, H, batch_first=True, bidirectional=len(layers) == 2).double()
    with torch.no_grad():
        for lay, sfx in zip(layers, ("", "_reverse")):
            getattr(ref, "weight_ih_l0" + sfx).copy_(lay.kernel.t())
            getattr(ref, "weight_hh_l0" + sfx).copy_(lay.recurrent.t())
            getattr(ref, "bias_ih_l0" + sfx).copy_(lay.bias)
            getattr(ref, "bias_hh_l0" + sfx).zero_()
    return ref


def _random_layer(D, H, seed, **kw):
    torch.manual_seed(seed)
    lay = L.KerasLSTM(D, H, impl="torch", **kw)
    with torch.no_grad():
        lay.bias.add_(0.1 * torch.randn(4 * H, dtype=torch.float64))      # away from its special initial value
    return lay


@pytest.mark.parametrize("B,T,D,H", [(3, 5, 7, 8), (5, 25, 256, 128)])
@pytest.mark.parametrize("go_backwards", [False, True])
def test_torch_impl_against_nn_lstm_and_numpy_forward_and_all_gradients(B, T, D, H, go_backwards):
    lay = _random_layer(D, H, 0, return_sequences=True, go_backwards=go_backwards).eval()
    x = torch.randn(B, T, D, dtype=torch.float64, requires_grad=True)
    wts = torch.randn(B, T, H, dtype=torch.float64) / (B * T) ** 0.5      # the loss: sum(h_seq * wts), gradients of order one
    h = lay(x)
    (h * wts).sum().backward()
    got = dict(h=h.detach().numpy(), dx=x.grad.numpy(), dkernel=lay.kernel.grad.numpy(), drecurrent=lay.recurrent.grad.numpy(),
               dbias=lay.bias.grad.numpy())

    # torch.nn.LSTM on the reversed input is the layer that goes backwards
    ref = _nn_lstm([lay], D, H)
    xr = x.detach().clone().requires_grad_(True)
    hr, _ = ref(xr.flip(1) if go_backwards else xr)
    (hr * wts).sum().backward()
    want = dict(h=hr.detach().numpy(), dx=xr.grad.numpy(), dkernel=ref.weight_ih_l0.grad.t().numpy(), drecurrent=ref.weight_hh_l0.grad.t().numpy(),
                dbias=ref.bias_ih_l0.grad.numpy())
    for k in got:
        err = float(np.abs(got[k] - want[k]).max())
        assert err < TOL, ("nn.LSTM", k, err)

    p = [lay.kernel.detach().numpy(), lay.recurrent.detach().numpy(), lay.bias.detach().numpy()]
    fw = npl.forward(*p, x.detach().numpy(), go_backwards=go_backwards)
    bw = npl.backward(p[0], p[1], fw, wts.numpy(), go_backwards=go_backwards)
    want = dict(h=fw["h_seq"], dx=bw["dx"], dkernel=bw["dkernel"], drecurrent=bw["drecurrent"], dbias=bw["dbias"])
    for k in got:
        err = float(np.abs(got[k] - want[k]).max())
        assert err < TOL, ("numpy", k, err)


def test_recurrence_with_an_initial_state_against_numpy():
    """lstm_recurrence_torch is the GPU tests' yardstick, initial state included (the layer itself always starts from zeros)"""
    rng = np.random.default_rng(3)
    B, T, D, H = 4, 3, 5, 8
    k, u, b = rng.standard_normal((D, 4 * H)) * 0.3, rng.standard_normal((H, 4 * H)) * 0.3, rng.standard_normal(4 * H) * 0.1
    x, h0, c0 = rng.standard_normal((B, T, D)), rng.standard_normal((B, H)) * 0.5, rng.standard_normal((B, H))
    fw = npl.forward(k, u, b, x, h0=h0, c0=c0)
    t = torch.tensor
    hs, cs = L.lstm_recurrence_torch(t(x) @ t(k) + t(b), t(u), t(h0), t(c0))
    assert np.abs(hs.numpy() - fw["h_seq"]).max() < TOL and np.abs(cs.numpy() - fw["c_seq"]).max() < TOL


def test_direction_semantics_against_bidirectional_nn_lstm():
    B, T, D, H = 4, 6, 5, 8
    x = torch.randn(B, T, D, dtype=torch.float64)
    for seq in (False, True):
        f = _random_layer(D, H, 1, return_sequences=seq)
        b = _random_layer(D, H, 2, return_sequences=seq, go_backwards=True)
        bi = L.KerasBidirectional(f, b).eval()
        with torch.no_grad():
            out, _ = _nn_lstm([f, b], D, H)(x)          # [B, T, 2H] in time order: [:, t, :H] forward, [:, t, H:] backward
            got = bi(x)
            if seq:
                assert got.shape == (B, T, 2 * H)
                assert float((got - out).abs().max()) < TOL            # [fwd, bwd], the backward half back in time order
                assert float((b(x) - out[:, :, H:].flip(1)).abs().max()) < TOL      # the member alone: consumption order
            else:
                assert got.shape == (B, 2 * H)
                assert float((got[:, :H] - out[:, -1, :H]).abs().max()) < TOL       # forward member: the state after x[T-1]
                assert float((got[:, H:] - out[:, 0, H:]).abs().max()) < TOL        # backward member: the state after x[0]
                assert float((f(x) - out[:, -1, :H]).abs().max()) < TOL and float((b(x) - out[:, 0, H:]).abs().max()) < TOL


def test_initialisers():
    torch.manual_seed(5)
    lay = L.KerasLSTM(256, 128)
    assert lay.kernel.shape == (256, 512) and lay.recurrent.shape == (128, 512) and lay.bias.shape == (512,)
    assert all(p.dtype == torch.float64 for p in lay.parameters())
    b = lay.bias.detach()
    assert bool((b[128:256] == 1).all()) and bool((b[:128] == 0).all()) and bool((b[256:] == 0).all())
    u = lay.recurrent.detach()
    assert float((u @ u.t() - torch.eye(128, dtype=torch.float64)).abs().max()) < 1e-12
    limit = (6.0 / (256 + 512)) ** 0.5
    k = lay.kernel.detach()
    assert float(k.abs().max()) <= limit and float(k.abs().max()) > 0.99 * limit        # 131 072 uniform draws reach the edge
    assert abs(float(k.std()) - limit / 3 ** 0.5) < 0.01 * limit                        # uniform on [-limit, limit]


def test_dropout_one_mask_per_call_constant_over_time_absent_in_eval():
    B, T, D, H = 64, 4, 32, 8
    torch.manual_seed(6)
    lay = L.KerasLSTM(D, H, return_sequences=True, impl="torch")
    m = lay.dropout_mask(torch.zeros(B, T, D, dtype=torch.float64))
    assert m.shape == (B, 1, D)                                       # broadcast over t: the same mask at every step
    vals = set(m.unique().tolist())
    assert vals == {0.0, 1.0 / 0.7}                                   # kept inputs are scaled by 1 / 0.7
    assert abs(float((m > 0).double().mean()) - 0.7) < 0.05           # 2048 draws: sigma 0.01
    # the layer in training mode IS the layer in eval mode on x * mask, mask drawn from the same generator state
    x = torch.randn(B, T, D, dtype=torch.float64)
    lay.train()
    torch.manual_seed(7)
    got = lay(x)
    torch.manual_seed(7)
    mask = lay.dropout_mask(x)
    lay.eval()
    with torch.no_grad():
        assert float((lay(x * mask) - got).abs().max()) == 0.0
        assert float((lay(x) - got).abs().max()) > 1e-3               # eval: no mask
        assert float((lay(x) - lay(x)).abs().max()) == 0.0


def test_param_counts():
    """by hand from net/layers.py: an LSTM has 4H (D + H + 1) parameters; the nets' convs 4 736 + 98 560 + 196 864, conv BNs 768,
    dense 512 (in + 1) + 131 328 + 32 896 + 8 256 + 65 with in = 256 (BiLSTM) or 128, dense BNs 1 792"""
    cnt = lambda mod: sum(p.numel() for p in mod.parameters() if p.requires_grad)
    assert cnt(L.KerasLSTM(256, 128)) == 4 * 128 * (256 + 128 + 1) == 197120
    assert cnt(L.KerasLSTM(128, 128)) == 4 * 128 * (128 + 128 + 1) == 131584
    bi, ls = L.ConvBiLstmNet(), L.ConvLstmNet()
    assert cnt(bi.conv3) == 196864 and cnt(bi.fc1) == 131584 and cnt(ls.fc1) == 66048 and cnt(bi.lstm) == 2 * 197120
    assert cnt(bi) == 1001089
    assert cnt(ls) == 870017
    for m in (bi, ls):
        assert sum(b.numel() for n, b in m.named_buffers() if "running" in n) == 2560


@pytest.mark.parametrize("name", ["conv_bilstm", "conv_lstm"])
def test_shapes_and_train_step_lowers_the_loss(name):
    torch.manual_seed(0)
    m = L.make_model(name)
    x = torch.randn(16, 200, 12, dtype=torch.float64)
    m.eval()
    with torch.no_grad():
        out = m(x[:5])
    assert out.shape == (5, 1) and out.dtype == torch.float32
    y = 300 + 1100 * torch.rand(16)
    mean, std = cn.channel_stats(x)
    opt = cn.make_optimizer(m)
    losses = [float(cn.train_step(m, opt, x, y, mean, std)[0]) for _ in range(12)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_make_model_names_and_fallback():
    assert type(L.make_model("conv")) is cn.ConvNet
    assert type(L.make_model("conv_lstm")) is L.ConvLstmNet
    assert type(L.make_model("conv_bilstm")) is L.ConvBiLstmNet
    assert type(L.make_model("lstm")) is cn.ConvNet and type(L.make_model("anything else")) is cn.ConvNet


def test_impl_switch(monkeypatch):
    x = torch.zeros(2, 3, 4, dtype=torch.float64)
    monkeypatch.delenv("SG_LSTM_IMPL", raising=False)
    assert L.choose_impl("auto", x, 128) == "torch"                   # a CPU tensor
    assert L.choose_impl("hip", x, 128) == "hip" and L.choose_impl("torch", x, 128) == "torch"
    monkeypatch.setenv("SG_LSTM_IMPL", "hip")                         # read per call, over the layer's own choice
    assert L.choose_impl("torch", x, 128) == "hip"
    lay = L.KerasLSTM(4, 128, impl="torch").eval()
    with pytest.raises(ValueError, match="HIP device"):               # forced and unable to run: an error, no fall-back
        lay(x)
    monkeypatch.setenv("SG_LSTM_IMPL", "torch")
    assert L.choose_impl("hip", x, 128) == "torch" and lay(x).shape == (2, 128)
    monkeypatch.setenv("SG_LSTM_IMPL", "fast")
    with pytest.raises(ValueError):
        L.choose_impl("auto", x, 128)
    monkeypatch.delenv("SG_LSTM_IMPL")
    with pytest.raises(ValueError, match="H = 128"):
        L.KerasLSTM(4, 8, impl="hip").eval()(x)


def test_invalid_arguments_are_refused_before_the_device():
    from softgrip_amd import native
    lib = native.lib()
    INV = native.SG_ERR_INVALID
    d = C.c_void_p(8)      # never dereferenced: the argument checks come first
    fwd = lambda B=4, T=3, H=128, z=d, U=d, c_seq=d, save=1: lib.sg_lstm_forward(B, T, H, z, U, None, None, None, None, None, c_seq, save, None)
    bwd = lambda B=4, T=3, H=128, gates=d, c_seq=d, U=d, dz=d: lib.sg_lstm_backward(B, T, H, gates, c_seq, None, U, None, None, dz, None, None, None)
    cases = [("sg_lstm_forward", fwd, [dict(B=0), dict(B=-1), dict(T=0), dict(H=64), dict(H=256), dict(z=None), dict(U=None), dict(c_seq=None)]),
             ("sg_lstm_backward", bwd, [dict(B=0), dict(T=-2), dict(H=127), dict(gates=None), dict(c_seq=None), dict(U=None), dict(dz=None)])]
    for name, call, bad in cases:
        for kw in bad:
            assert call(**kw) == INV, (name, kw)
            msg = lib.sg_last_error()
            assert msg.startswith(name.encode() + b":") and len(msg) > len(name) + 2, (name, kw, msg)


def test_kept_assembly_no_scratch_no_spills_f64_mfma_one_workgroup_per_cu():
    """sg_lstm.device.s: both kernels 0 bytes of scratch and no spills, v_mfma_f64_16x16x4 in both; the register and LDS figures DESIGN.md
    9.3 quotes -- forward 32 KB of LDS (h, double-buffered), backward 64 KB (the dz tile) -- and within one wavefront's 512 registers"""
    import os
    import sys
    from softgrip_amd import build_native, devasm
    build_native.build()
    path = build_native.device_asm("sg_lstm.hip")
    # kept in the object directory's nn/ (build_native.SOURCE_SUBDIR), so not among device_asm_files(): the build's static check, again here
    assert os.path.basename(os.path.dirname(path)) == "nn" and path not in build_native.device_asm_files()
    sys.path.insert(0, os.path.dirname(os.path.abspath(build_native.__file__)))
    import isa_check
    assert isa_check.check_asm(path) == [], isa_check.describe(isa_check.check_asm(path), path)
    text = open(path).read()
    seen = devasm.kernels(text)
    fwd = [v for k, v in seen.items() if "sg_lstm_fwd_kernel" in k]
    bwd = [v for k, v in seen.items() if "sg_lstm_bwd_kernel" in k]
    assert len(fwd) == 1 and len(bwd) == 1 and len(seen) == 2, sorted(seen)
    for v in fwd + bwd:
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0, v
        assert v["agpr"] <= v["vgpr"] <= 512, v      # (the metadata's vgpr_count is the unified file's: architectural + accumulator)
    assert fwd[0]["lds"] == 2 * 16 * 128 * 8 and bwd[0]["lds"] == 16 * 512 * 8
    # workgroups per CU: a workgroup is 4 wavefronts = one per SIMD, and a SIMD holds 512 registers per lane: above 256 registers
    # one workgroup per CU whatever the LDS -- the grid is ceil(B / 16) <= 256 at the project's batch, one workgroup per CU anyway
    for v in fwd + bwd:
        assert min(512 // v["vgpr"], (160 * 1024) // v["lds"]) == 1, v
    funcs = devasm.functions(text)
    for key in ("sg_lstm_fwd_kernel", "sg_lstm_bwd_kernel"):
        body = [ins for name, lines in funcs.items() if key in name for _, ins in lines]
        n = sum(1 for ins in body if re.match(r"v_mfma_f64_16x16x4", ins))
        assert n >= 8, (key, n)
