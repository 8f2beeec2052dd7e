"""The fp64 LSTM kernels (csrc/sg_lstm.hip) and the recurrent regressors on the GPU.  The yardstick everywhere is the step loop in torch
ops (lstm.lstm_recurrence_torch, impl="torch") on the CPU in fp64 with the same weights and inputs; tests/test_lstm_host.py holds that
against torch.nn.LSTM and NumPy.  Every test prints what it measured."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from helpers import model_path
from softgrip_amd import convnet as cn
from softgrip_amd import lstm as L

pytestmark = pytest.mark.gpu

H, G = 128, 512
TOL_FWD = 1e-12        # absolute on h and c (|h| < 1, |c| < T)
TOL_BWD = 1e-10        # relative L2 per tensor
DEV = "cuda:0"


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).norm() / want.norm())


@functools.lru_cache(maxsize=None)
def _case(B, T, state=False, seed=0):
    """inputs of one direction and the yardstick's answers, computed once and shared (read-only): z, U (random, asymmetric), h0 / c0 when
    `state`, weights wseq / wlast of the two losses; h_seq, c_seq, gates; dz of sum(h_seq * wseq) and of sum(h_last * wlast)"""
    g = torch.Generator().manual_seed(1000 * B + 10 * T + seed)
    rn = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    z, U = rn(B, T, G), 0.15 * rn(H, G)
    h0, c0 = (torch.tanh(rn(B, H)), rn(B, H)) if state else (None, None)
    wseq, wlast = rn(B, T, H), rn(B, H)
    zr = z.clone().requires_grad_(True)
    hs, cs = L.lstm_recurrence_torch(zr, U, h0, c0)
    dz_seq, = torch.autograd.grad((hs * wseq).sum(), zr, retain_graph=True)
    dz_last, = torch.autograd.grad((hs[:, -1] * wlast).sum(), zr)
    hs, cs = hs.detach(), cs.detach()
    hp = torch.cat([(torch.zeros(B, 1, H, dtype=torch.float64) if h0 is None else h0[:, None]), hs[:, :-1]], dim=1)
    a = z + hp @ U
    gates = torch.cat([torch.sigmoid(a[..., :2 * H]), torch.tanh(a[..., 2 * H:3 * H]), torch.sigmoid(a[..., 3 * H:])], dim=-1)
    return dict(z=z, U=U, h0=h0, c0=c0, wseq=wseq, wlast=wlast, h_seq=hs, c_seq=cs, gates=gates, dz_seq=dz_seq, dz_last=dz_last)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def test_one_step_in_isolation_with_a_state_and_an_asymmetric_u():
    """T = 1 from random non-zero h0, c0: the one product h0 . U with nothing around it -- a wrong f64 MFMA lane map or a transposed U
    shows here (with zero h0 a single step never runs the product)"""
    k = _case(16, 1, state=True)
    assert float((k["U"][:, :H] - k["U"][:, :H].t()).abs().max()) > 0.1
    out = L.lstm_forward_hip(_dev(k["z"]), _dev(k["U"]), _dev(k["h0"]), _dev(k["c0"]), sequences=True, save=False)
    eh = float((out["h_last"].cpu() - k["h_seq"][:, 0]).abs().max())
    ec = float((out["c_last"].cpu() - k["c_seq"][:, 0]).abs().max())
    es = float((out["h_seq"].cpu() - k["h_seq"]).abs().max())
    print("one step: max |h - yardstick| = %.3e, |c - yardstick| = %.3e" % (eh, ec))
    assert eh < TOL_FWD and ec < TOL_FWD and es < TOL_FWD


@pytest.mark.parametrize("T", [2, 25])
@pytest.mark.parametrize("B", [1, 17, 100])
def test_forward_kernel_sequences_last_save_on_and_off(B, T):
    k = _case(B, T)
    U = _dev(k["U"])
    worst = 0.0
    for save in (False, True):
        for sequences in (False, True):
            z = _dev(k["z"])
            out = L.lstm_forward_hip(z, U, sequences=sequences, save=save)
            assert ("h_seq" in out) == (sequences or save) and ("c_seq" in out) == save
            errs = [float((out["h_last"].cpu() - k["h_seq"][:, -1]).abs().max()), float((out["c_last"].cpu() - k["c_seq"][:, -1]).abs().max())]
            if "h_seq" in out:
                errs.append(float((out["h_seq"].cpu() - k["h_seq"]).abs().max()))
            if save:
                errs.append(float((out["c_seq"].cpu() - k["c_seq"]).abs().max()))
                errs.append(float((z.cpu() - k["gates"]).abs().max()))          # z now holds the activated gates
            else:
                assert torch.equal(z.cpu(), k["z"])                              # untouched
            worst = max(worst, *errs)
            assert max(errs) < TOL_FWD, (save, sequences, errs)
    print("forward kernel B=%d T=%d: max abs error on h, c, gates = %.3e" % (B, T, worst))


@pytest.mark.parametrize("T", [2, 25])
@pytest.mark.parametrize("B", [1, 17, 100])
def test_layer_both_directions_sequences_and_last(B, T):
    torch.manual_seed(B + T)
    x = torch.randn(B, T, 256, dtype=torch.float64)
    worst = 0.0
    for back in (False, True):
        for seq in (False, True):
            ref = L.KerasLSTM(256, H, return_sequences=seq, go_backwards=back, impl="torch").eval()
            with torch.no_grad():
                ref.recurrent.copy_(0.15 * torch.randn(H, G, dtype=torch.float64))     # asymmetric, not orthogonal
            dev = copy.deepcopy(ref).to(DEV)
            dev.impl = "hip"
            with torch.no_grad():
                want, got = ref(x), dev(x.to(DEV))
            assert got.shape == want.shape and got.is_cuda and got.dtype == torch.float64
            err = float((got.cpu() - want).abs().max())
            worst = max(worst, err)
            assert err < TOL_FWD, (back, seq, err)
    print("layer B=%d T=%d: max |h - yardstick| = %.3e" % (B, T, worst))


def _raw(name, *args):
    from softgrip_amd import native
    lib = native.lib()
    p = lambda a: a if isinstance(a, int) else None if a is None else C.c_void_p(a.data_ptr())
    native.check(getattr(lib, name)(*[p(a) for a in args], C.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)


SENTINEL = -7.25


def test_tile_tails_sentinels_batch_independence_and_repeatability():
    """B = 17 ends one row into its second 16-row tile: the 15 rows after it are neither read into results nor written; a row's result
    does not depend on B; two identical calls give identical bits -- forward and backward"""
    T = 3
    big = _case(100, T)
    n, pad = 17, 15

    def run(B, rows):
        buf = lambda *s: torch.full((rows,) + s, SENTINEL, dtype=torch.float64, device=DEV)
        o = dict(z=buf(T, G), h_seq=buf(T, H), h_last=buf(H), c_last=buf(H), c_seq=buf(T, H), dz=buf(T, G), dh0=buf(H), dc0=buf(H))
        o["z"][:B] = big["z"][:B].to(DEV)
        U = _dev(big["U"])
        _raw("sg_lstm_forward", B, T, H, o["z"], U, None, None, o["h_seq"], o["h_last"], o["c_last"], o["c_seq"], 1)
        dh_seq, dh_last = _dev(big["wseq"][:B]), _dev(big["wlast"][:B])
        _raw("sg_lstm_backward", B, T, H, o["z"], o["c_seq"], None, U, dh_seq, dh_last, o["dz"], o["dh0"], o["dc0"])
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in o.items()}

    a = run(n, n + pad)
    for k, v in a.items():
        assert bool((v[n:] == SENTINEL).all()), "sentinel rows of %s were written" % k
        assert bool(torch.isfinite(v[:n]).all()) and not bool((v[:n] == SENTINEL).all()), k
    again = run(n, n + pad)
    full = run(100, 100)
    for k, v in a.items():
        assert torch.equal(v, again[k]), "two identical calls differ in %s" % k
        assert torch.equal(v[:n], full[k][:n]), "rows 0-16 of %s depend on B" % k
    assert float((full["h_seq"] - big["h_seq"]).abs().max()) < TOL_FWD
    want_dz = big["dz_seq"] + big["dz_last"]
    print("tails: relative L2 error of dz at B=100, T=3, both gradients flowing in = %.3e" % _rel(full["dz"], want_dz))
    assert _rel(full["dz"], want_dz) < TOL_BWD


@pytest.mark.parametrize("B,T", [(17, 3), (100, 25)])
@pytest.mark.parametrize("sequences", [False, True])
def test_backward_kernel_dz_and_state_gradients(B, T, sequences):
    k = _case(B, T, state=True)
    U, h0, c0 = _dev(k["U"]), _dev(k["h0"]), _dev(k["c0"])
    z = _dev(k["z"])
    out = L.lstm_forward_hip(z, U, h0, c0, save=True)
    dz, dh0, dc0 = L.lstm_backward_hip(z, out["c_seq"], U, dh_seq=_dev(k["wseq"]) if sequences else None,
                                       dh_last=None if sequences else _dev(k["wlast"]), c0=c0, state_grads=True)
    want = k["dz_seq"] if sequences else k["dz_last"]
    # the state gradients from the yardstick's graph
    zr, hr, cr = k["z"].clone().requires_grad_(True), k["h0"].clone().requires_grad_(True), k["c0"].clone().requires_grad_(True)
    hs, _ = L.lstm_recurrence_torch(zr, k["U"], hr, cr)
    wdh0, wdc0 = torch.autograd.grad((hs * k["wseq"]).sum() if sequences else (hs[:, -1] * k["wlast"]).sum(), (hr, cr))
    errs = dict(dz=_rel(dz, want), dh0=_rel(dh0, wdh0), dc0=_rel(dc0, wdc0))
    print("backward kernel B=%d T=%d %s: relative L2 errors %s" % (B, T, "sequences" if sequences else "last", errs))
    assert max(errs.values()) < TOL_BWD, errs


@pytest.mark.parametrize("B,T", [(17, 3), (100, 25)])
@pytest.mark.parametrize("sequences", [False, True])
@pytest.mark.parametrize("back", [False, True])
def test_autograd_function_gradients_against_cpu_autograd(B, T, sequences, back):
    torch.manual_seed(10 * B + T)
    D = 256
    ref = L.KerasLSTM(D, H, return_sequences=sequences, go_backwards=back, impl="torch").eval()
    with torch.no_grad():
        ref.bias.add_(0.1 * torch.randn(G, dtype=torch.float64))
    dev = copy.deepcopy(ref).to(DEV)
    dev.impl = "hip"
    x = torch.randn(B, T, D, dtype=torch.float64)
    w = torch.randn((B, T, H) if sequences else (B, H), dtype=torch.float64)
    xr, xd = x.clone().requires_grad_(True), x.to(DEV).requires_grad_(True)
    (ref(xr) * w).sum().backward()
    (dev(xd) * w.to(DEV)).sum().backward()
    errs = dict(dx=_rel(xd.grad, xr.grad), dkernel=_rel(dev.kernel.grad, ref.kernel.grad), drecurrent=_rel(dev.recurrent.grad, ref.recurrent.grad),
                dbias=_rel(dev.bias.grad, ref.bias.grad))
    print("autograd B=%d T=%d seq=%s back=%s: relative L2 errors %s" % (B, T, sequences, back, errs))
    assert max(errs.values()) < TOL_BWD, errs


def test_auto_picks_the_kernels_on_the_gpu_and_a_forced_hip_refuses_float32(monkeypatch):
    monkeypatch.delenv("SG_LSTM_IMPL", raising=False)
    x = torch.zeros(2, 3, 4, dtype=torch.float64, device=DEV)
    assert L.choose_impl("auto", x, 128) == "hip" and L.choose_impl("auto", x, 64) == "torch" and L.choose_impl("auto", x.float(), 128) == "torch"
    with pytest.raises(ValueError, match="float64"):
        L.lstm_forward_hip(torch.zeros(2, 3, G, device=DEV), torch.zeros(H, G, device=DEV))


def _randomised(net):
    with torch.no_grad():   # moving statistics and biases away from their initial values, so that inference mode tests something
        for name, b in net.named_buffers():
            b.copy_(0.05 * torch.randn(b.shape) if name.endswith("mean") else 0.8 + 0.4 * torch.rand(b.shape))
        for name, p in net.named_parameters():
            if name.endswith("bias") and p.dtype == torch.float32:
                p.copy_(0.05 * torch.randn(p.shape))
    return net


@pytest.mark.parametrize("name", ["conv_bilstm", "conv_lstm"])
def test_nets_eval_forward_against_the_cpu_at_batch_100(name):
    """the gate is test_regressor_step_numerics_at_full_size's for the float32 convs and dense layers (1e-4 of the head's range on the
    predictions, against an fp64 evaluation on the CPU); the fp64 LSTM adds nothing to it"""
    torch.manual_seed(2)
    net = _randomised(L.make_model(name))
    ref = copy.deepcopy(net).double().eval()
    x = torch.randn(100, 200, 12, dtype=torch.float64)
    net = net.to(DEV).eval()
    for m in net.modules():
        if isinstance(m, L.KerasLSTM):
            m.impl = "hip"
    with torch.no_grad():
        got = cn.normalize_predictions(net(x.to(DEV))).cpu().double()
        want = cn.normalize_predictions(ref(x))
    err = float((got - want).abs().max())
    print("%s eval forward at B=100: max |pred - fp64 CPU| = %.3e (head range 300 .. 1400)" % (name, err))
    assert got.shape == (100,) and err < 1e-4 * 1400


@pytest.mark.parametrize("name", ["conv_bilstm", "conv_lstm"])
def test_nets_train_step_hip_against_torch_ops_and_five_steps_lower_the_loss(name):
    """one training step with the kernels and one with the torch step loop, both on the GPU, from the same weights, batch and dropout
    masks (the same generator state): the float32 layers around the LSTM see the same numbers unless a difference of 1e-16 crosses a
    float32 rounding boundary, so losses and gradients agree within the backward tolerance"""
    torch.manual_seed(3)
    base = L.make_model(name).to(DEV)
    x = torch.randn(100, 200, 12, dtype=torch.float64, device=DEV)
    y = (300 + 1100 * torch.rand(100)).to(DEV)
    mean, std = cn.channel_stats(x)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True        # the convolutions' weight gradients: the same algorithm, the same order, both times
    try:
        res = {}
        for impl in ("hip", "torch"):
            net = copy.deepcopy(base)
            for m in net.modules():
                if isinstance(m, L.KerasLSTM):
                    m.impl = impl
            opt = cn.make_optimizer(net)
            torch.manual_seed(11)
            loss, _ = cn.train_step(net, opt, x, y, mean, std)
            res[impl] = (float(loss), {k: p.grad.detach().clone() for k, p in net.named_parameters()}, net, opt)
    finally:
        torch.backends.cudnn.deterministic = was
    (lh, gh, net, opt), (lt, gt, _, _) = res["hip"], res["torch"]
    errs = {k: (_rel(gh[k], gt[k]) if float(gt[k].norm()) > 0 else float(gh[k].norm())) for k in gt}
    worst = max(errs, key=errs.get)
    print("%s train step: loss hip %.12g, torch ops %.12g; worst gradient %s relative L2 %.3e" % (name, lh, lt, worst, errs[worst]))
    assert abs(lh - lt) <= TOL_BWD * abs(lt)
    assert errs[worst] < TOL_BWD, {k: v for k, v in errs.items() if v >= TOL_BWD}
    losses = [lh] + [float(cn.train_step(net, opt, x, y, mean, std)[0]) for _ in range(5)]
    print("%s losses over the steps: %s" % (name, ["%.2f" % v for v in losses]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_episode_block_into_a_bilstm_train_step_without_leaving_the_gpu():
    from softgrip_amd import ManEnv
    from softgrip_amd.create_dataset import episode_schedule
    np.random.seed(2)
    n = 64
    env = ManEnv(1, 7, [model_path("softbox")], is_vis=False, n_envs=n)
    env.set_new_stiffness()
    out, flags = env.rollout(episode_schedule())
    assert out.shape == (n, 200, 12) and out.is_cuda and out.dtype == torch.float64 and int((flags != 0).sum()) == 0
    torch.manual_seed(0)
    net = L.ConvBiLstmNet(impl="hip").to(out.device)
    opt = cn.make_optimizer(net)
    y = torch.tensor(env.stiffness, device=out.device)
    mean, std = cn.channel_stats(out)
    loss, pred = cn.train_step(net, opt, out, y, mean, std, add_noise=True)
    assert pred.is_cuda and pred.shape == (n,) and bool(torch.isfinite(loss)) and bool(torch.isfinite(pred).all())
    assert float(pred.min()) >= 300 and float(pred.max()) <= 1400
    print("end to end: loss %.2f, predictions %.1f .. %.1f" % (float(loss), float(pred.min()), float(pred.max())))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
