"""One BiLSTM layer (256 -> 2 x 128, fp64, last state out, no dropout) timed with HIP events on the GPU, three implementations in the same
run on the same inputs, each forward-only (no_grad) and forward + backward (loss = sum of the output):

  hip        soft-grip_amd/lstm.py with impl="hip": the input projection and the weight gradients in rocBLAS, the recurrence in
             csrc/sg_lstm.hip (one kernel per direction and pass)
  torch_ops  the same layer with impl="torch": the step loop in torch ops
  nn_lstm    torch.nn.LSTM(256, 128, bidirectional=True, batch_first=True).double() carrying the same weights -- the yardstick

at (B, T, D) = (100, 25, 256), the reference's batch, and (4096, 25, 256), this project's.  Each figure is the median of `rounds`
windows of `reps` back-to-back calls between two events, after a warm-up call; the implementations' windows alternate.  Also timed
alone, the same way: the forward kernel (with and without saving) and the backward kernel of one direction, from which the L2 read
rate the streaming of U implies is derived (ceil(B / 16) workgroups x T steps x 512 KB per kernel).

usage: python scripts/lstm_bench.py [--reps 10] [--rounds 5] [--out profiles/r13_lstm_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_lstm_bench.json"))
    args = ap.parse_args()
    import torch
    from softgrip_amd import lstm as L
    dev = torch.device("cuda", 0)
    D, H = 256, 128
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, rounds=args.rounds, unit="ms per call (median window / reps)", sizes=[])
    for B, T in ((100, 25), (4096, 25)):
        torch.manual_seed(0)
        layers = {}
        for impl in ("hip", "torch"):
            torch.manual_seed(1)
            layers[impl] = L.KerasBidirectional(L.KerasLSTM(D, H, dropout=0.0, impl=impl), L.KerasLSTM(D, H, go_backwards=True, dropout=0.0, impl=impl)).to(dev)
        ref = torch.nn.LSTM(D, H, batch_first=True, bidirectional=True).double().to(dev)
        with torch.no_grad():
            for lay, sfx in ((layers["hip"].fwd, ""), (layers["hip"].bwd, "_reverse")):
                getattr(ref, "weight_ih_l0" + sfx).copy_(lay.kernel.t())
                getattr(ref, "weight_hh_l0" + sfx).copy_(lay.recurrent.t())
                getattr(ref, "bias_ih_l0" + sfx).copy_(lay.bias)
                getattr(ref, "bias_hh_l0" + sfx).zero_()
        x = torch.randn(B, T, D, dtype=torch.float64, device=dev)

        def nn_out(x):
            out, _ = ref(x)
            return torch.cat([out[:, -1, :H], out[:, 0, H:]], dim=-1)

        models = dict(hip=(layers["hip"], layers["hip"]), torch_ops=(layers["torch"], layers["torch"]), nn_lstm=(nn_out, ref))

        def fwd_only(f):
            def run():
                with torch.no_grad():
                    f(x)
            return run

        def fwd_bwd(f, mod):
            def run():
                mod.zero_grad(set_to_none=True)
                f(x).sum().backward()
            return run

        with torch.no_grad():       # the three compute the same thing
            outs = {k: f(x) for k, (f, _) in models.items()}
        agree = {k: float((outs[k] - outs["nn_lstm"]).abs().max()) for k in outs}

        cases = {}
        for k, (f, mod) in models.items():
            cases[k + " forward"] = fwd_only(f)
            cases[k + " forward+backward"] = fwd_bwd(f, mod)
        # the kernels of one direction alone
        z = torch.randn(B, T, 4 * H, dtype=torch.float64, device=dev)
        U = layers["hip"].fwd.recurrent.detach().contiguous()
        saved = L.lstm_forward_hip(z.clone(), U, save=True)
        gates = z.clone()
        L.lstm_forward_hip(gates, U, save=True)
        dh = torch.randn(B, T, H, dtype=torch.float64, device=dev)
        zs = z.clone()
        cases["kernel forward (no save, last state only)"] = lambda: L.lstm_forward_hip(z, U, sequences=False, save=False)
        cases["kernel forward (save)"] = lambda: L.lstm_forward_hip(zs, U, save=True)      # (re-activates its own output: same work)
        cases["kernel backward"] = lambda: L.lstm_backward_hip(gates, saved["c_seq"], U, dh_seq=dh)

        for fn in cases.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(args.rounds):
            for k, fn in cases.items():
                times[k].append(window(torch, fn, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        u_bytes = -(-B // 16) * T * H * 4 * H * 8
        entry = dict(B=B, T=T, D=D, H=H, ms=med, windows_ms=times, max_abs_difference_from_nn_lstm=agree,
                     U_stream_bytes_per_kernel=u_bytes,
                     implied_L2_read_GBps=dict(forward=u_bytes / (med["kernel forward (no save, last state only)"] * 1e-3) / 1e9,
                                               backward=u_bytes / (med["kernel backward"] * 1e-3) / 1e9))
        result["sizes"].append(entry)
        print("B=%d T=%d" % (B, T))
        for k, v in med.items():
            print("  %-45s %9.4f ms" % (k, v))
        print("  agreement with nn.LSTM (max abs): %s" % agree)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for e in result["sizes"] for k, v in [("B%d" % e["B"], e["ms"])]}))


if __name__ == "__main__":
    main()
