"""The reference's two recurrent stiffness regressors (net/NeuralNets.py:30-80, net/layers.py:4-10) in PyTorch-ROCm, on an fp64 LSTM
layer whose recurrence runs in one HIP kernel per direction (csrc/sg_lstm.hip): ConvBiLstmNet -- the reference's default model -- and
ConvLstmNet.  Both consume the simulator's on-device ``[n, 200, 12]`` observation block like convnet.ConvNet and reuse its batch norm,
padding, head, statistics, optimiser and training step.  Restated from Keras' documented behaviour; nothing is copied.

The layer (tf.keras.layers.LSTM as the reference builds it: ``dtype=float64, dropout=0.3``, everything else Keras' default):
  kernel [D, 4H] Glorot uniform, recurrent [H, 4H] orthogonal (orthonormal rows), bias [4H] zeros with the forget block [H:2H] at one
  (unit_forget_bias); gate order i, f, c~, o along 4H -- torch's i, f, g, o; sigmoid on i, f, o and tanh on c~ and the cell; zero
  initial state; fp64 throughout, inputs cast at the layer's door (Keras autocast).
  go_backwards consumes x[:, T-1 .. 0]; the outputs come in consumption order.  KerasBidirectional turns the backward member's
  sequence back into time order and concatenates [fwd, bwd] on the feature axis.
  Input dropout, training only: ONE Bernoulli(0.7) mask [B, 1, D] per call, scaled by 1 / 0.7, the same at every time step, applied
  to x before the input product; no recurrent dropout.  (Keras' documented rule for ``dropout=``; unpinned here)

Two implementations of the recurrence behind one switch (``impl``; SG_LSTM_IMPL=torch|hip, read per call, forces one):
  torch  the step loop in torch ops: differentiable by autograd, any device, any H -- the CPU path and the kernels' yardstick
  hip    a torch.autograd.Function over sg_lstm_forward / sg_lstm_backward: H == 128, fp64, a HIP device.  The input projection for all
         steps (one GEMM) and the weight gradients (GEMMs over the stored sequences) stay in torch; the kernels do what is serial in
         time.  Forced and unable to run, it raises: there is no quiet fall-back.
  auto   hip exactly when its conditions hold and the library loads, torch otherwise (the default)
"""
import ctypes as C
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .convnet import ConvNet, KerasBatchNorm

HIP_HIDDEN = 128      # the H the kernels are built for


def lstm_recurrence_torch(z, U, h0=None, c0=None):
    """the recurrence in torch ops.  z [B, T, 4H]: x.kernel + bias in consumption order, U [H, 4H], h0 / c0 [B, H] or None (zeros)
    -> h_seq, c_seq [B, T, H]"""
    B, T, G = z.shape
    H = G // 4
    h = z.new_zeros(B, H) if h0 is None else h0
    c = z.new_zeros(B, H) if c0 is None else c0
    hs, cs = [], []
    for t in range(T):
        a = z[:, t] + h @ U
        i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
    return torch.stack(hs, dim=1), torch.stack(cs, dim=1)


def _lib():
    from . import native
    return native, native.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _check_hip(H, *tensors):
    if H != HIP_HIDDEN:
        raise ValueError("the HIP LSTM kernels are built for H = %d, not %d" % (HIP_HIDDEN, H))
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("the HIP LSTM kernels take contiguous float64 tensors on a HIP device (got %s, %s, contiguous=%s)"
                             % (t.device, t.dtype, t.is_contiguous()))


def lstm_forward_hip(z, U, h0=None, c0=None, sequences=True, save=False):
    """sg_lstm_forward on z [B, T, 4H] (overwritten with the activated gates when save) -> dict of h_seq (when sequences or save), h_last,
    c_last and, when save, c_seq"""
    B, T, G = z.shape
    _check_hip(G // 4, z, U, h0, c0)
    native, L = _lib()
    H = G // 4
    out = dict(h_last=z.new_empty(B, H), c_last=z.new_empty(B, H))
    if sequences or save:
        out["h_seq"] = z.new_empty(B, T, H)
    if save:
        out["c_seq"] = z.new_empty(B, T, H)
    with torch.cuda.device(z.device):
        native.check(L.sg_lstm_forward(B, T, H, _p(z), _p(U), _p(h0), _p(c0), _p(out.get("h_seq")), _p(out["h_last"]), _p(out["c_last"]),
                                       _p(out.get("c_seq")), int(save), _stream(z)), L)
    return out


def lstm_backward_hip(gates, c_seq, U, dh_seq=None, dh_last=None, c0=None, state_grads=False):
    """sg_lstm_backward -> dz [B, T, 4H] (and dh0, dc0 with state_grads)"""
    B, T, G = gates.shape
    _check_hip(G // 4, gates, c_seq, U, dh_seq, dh_last, c0)
    native, L = _lib()
    dz = torch.empty_like(gates)
    dh0 = gates.new_empty(B, G // 4) if state_grads else None
    dc0 = gates.new_empty(B, G // 4) if state_grads else None
    with torch.cuda.device(gates.device):
        native.check(L.sg_lstm_backward(B, T, G // 4, _p(gates), _p(c_seq), _p(c0), _p(U), _p(dh_seq), _p(dh_last), _p(dz), _p(dh0), _p(dc0),
                                        _stream(gates)), L)
    return (dz, dh0, dc0) if state_grads else dz


class _LstmHip(torch.autograd.Function):
    """x [B, T, D] (consumption order, dropout applied), kernel, recurrent, bias -> h_seq [B, T, H]"""

    @staticmethod
    def forward(ctx, x, kernel, recurrent, bias):
        B, T, D = x.shape
        z = torch.addmm(bias, x.reshape(B * T, D), kernel).view(B, T, -1)      # the input projection of all steps: one GEMM
        U = recurrent.contiguous()
        save = any(ctx.needs_input_grad)
        out = lstm_forward_hip(z, U, sequences=True, save=save)
        if save:
            ctx.save_for_backward(x, kernel, U, z, out["c_seq"], out["h_seq"])     # z now holds the gates
        return out["h_seq"]

    @staticmethod
    def backward(ctx, dh_seq):
        x, kernel, U, gates, c_seq, h_seq = ctx.saved_tensors
        B, T, D = x.shape
        H = U.shape[0]
        dz = lstm_backward_hip(gates, c_seq, U, dh_seq=dh_seq.contiguous())
        dz2 = dz.view(B * T, 4 * H)
        dx = (dz2 @ kernel.t()).view(B, T, D) if ctx.needs_input_grad[0] else None
        dkernel = _sum_outer(x, dz) if ctx.needs_input_grad[1] else None
        drec = None
        if ctx.needs_input_grad[2]:
            h_prev = torch.zeros_like(h_seq)          # h before step t: h_seq[t - 1], and the zero initial state at t = 0
            h_prev[:, 1:] = h_seq[:, :-1]
            drec = _sum_outer(h_prev, dz)
        dbias = dz2.sum(dim=0) if ctx.needs_input_grad[3] else None
        return dx, dkernel, drec, dbias


def _sum_outer(a, b):
    """sum over (batch, time) of a[b, t, :, None] * b[b, t, None, :]: a [B, T, M], b [B, T, N] -> [M, N].  As ONE GEMM this is a product
    with a small result (256 x 512) and a very long sum (B T = 102 400 at 4096): two output tiles, two busy CUs -- 45 ms per layer call at
    4096 when it was written so.  Split over up to 128 groups of batch rows it is a batched GEMM that fills the chip, and a sum of the
    partial results; the order is fixed, so two runs give the same bits."""
    B, T, M = a.shape
    S = math.gcd(B, 128)
    part = torch.bmm(a.reshape(S, (B // S) * T, M).transpose(1, 2), b.reshape(S, (B // S) * T, b.shape[2]))
    return part.sum(dim=0)


def hip_available():
    """the library is there and loads"""
    try:
        _lib()
        return True
    except (ImportError, OSError):
        return False


def choose_impl(impl, x, hidden):
    """'torch' or 'hip' for one call: SG_LSTM_IMPL over the layer's ``impl`` over auto's rule"""
    forced = os.environ.get("SG_LSTM_IMPL", "")
    if forced:
        if forced not in ("torch", "hip"):
            raise ValueError("SG_LSTM_IMPL must be torch or hip, not %r" % forced)
        impl = forced
    if impl not in ("auto", "torch", "hip"):
        raise ValueError("impl must be auto, torch or hip, not %r" % (impl,))
    if impl == "auto":
        return "hip" if (x.is_cuda and x.dtype == torch.float64 and hidden == HIP_HIDDEN and hip_available()) else "torch"
    return impl


class KerasLSTM(nn.Module):
    def __init__(self, input_size, hidden, return_sequences=False, go_backwards=False, dropout=0.3, impl="auto"):
        super().__init__()
        self.input_size, self.hidden = input_size, hidden
        self.return_sequences, self.go_backwards, self.dropout, self.impl = return_sequences, go_backwards, dropout, impl
        self.kernel = nn.Parameter(torch.empty(input_size, 4 * hidden, dtype=torch.float64))
        self.recurrent = nn.Parameter(torch.empty(hidden, 4 * hidden, dtype=torch.float64))
        self.bias = nn.Parameter(torch.zeros(4 * hidden, dtype=torch.float64))
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            limit = math.sqrt(6.0 / (self.input_size + 4 * self.hidden))        # Glorot uniform over (fan_in, fan_out) = (D, 4H)
            self.kernel.uniform_(-limit, limit)
            # Keras' Orthogonal on [H, 4H]: QR of a normal [4H, H] matrix, signs from R's diagonal, transposed -> orthonormal rows
            qm, rm = torch.linalg.qr(torch.randn(4 * self.hidden, self.hidden, dtype=torch.float64))
            self.recurrent.copy_((qm * torch.sign(torch.diagonal(rm))).t())
            self.bias.zero_()
            self.bias[self.hidden:2 * self.hidden] = 1.0                        # unit_forget_bias

    def dropout_mask(self, x):
        """[B, 1, D]: 0 or 1 / keep, one draw per call"""
        keep = 1.0 - self.dropout
        return torch.bernoulli(torch.full((x.shape[0], 1, x.shape[2]), keep, dtype=x.dtype, device=x.device)) / keep

    def forward(self, x):
        """x [B, T, D], any float dtype -> [B, T, H] in consumption order (return_sequences) or the last state [B, H]; float64"""
        x = x.to(self.kernel.dtype)
        if self.training and self.dropout > 0:
            x = x * self.dropout_mask(x)
        if self.go_backwards:
            x = x.flip(1)
        if choose_impl(self.impl, x, self.hidden) == "hip":
            _check_hip(self.hidden, self.kernel.detach(), self.recurrent.detach(), self.bias.detach())
            h_seq = _LstmHip.apply(x.contiguous(), self.kernel, self.recurrent, self.bias)
        else:
            h_seq, _ = lstm_recurrence_torch(x @ self.kernel + self.bias, self.recurrent)
        return h_seq if self.return_sequences else h_seq[:, -1]


class KerasBidirectional(nn.Module):
    """tf.keras.layers.Bidirectional(fwd, backward_layer=bwd), merge_mode "concat" """

    def __init__(self, fwd, bwd):
        super().__init__()
        assert not fwd.go_backwards and bwd.go_backwards and fwd.return_sequences == bwd.return_sequences
        self.fwd, self.bwd = fwd, bwd

    def forward(self, x):
        a, b = self.fwd(x), self.bwd(x)
        if self.bwd.return_sequences:
            b = b.flip(1)                   # back into time order
        return torch.cat([a, b], dim=-1)


class _ConvRecurrentNet(nn.Module):
    """what the two nets share: conv 128/256/256 (kernel 3, stride 2, SAME; BN + ReLU after the first two), the recurrent block in
    fp64, Dense 512/256/128 (+BN+ReLU each), Dense 64, Dense 1.  No pooling: `call` never uses the pooling layer it builds."""

    def __init__(self, recurrent_out, in_channels=12):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv1d(in_channels, 128, 3, stride=2), KerasBatchNorm(128)
        self.conv2, self.bn2 = nn.Conv1d(128, 256, 3, stride=2), KerasBatchNorm(256)
        self.conv3 = nn.Conv1d(256, 256, 3, stride=2)
        self.fc1, self.fbn1 = nn.Linear(recurrent_out, 512), KerasBatchNorm(512)
        self.fc2, self.fbn2 = nn.Linear(512, 256), KerasBatchNorm(256)
        self.fc3, self.fbn3 = nn.Linear(256, 128), KerasBatchNorm(128)
        self.fc4 = nn.Linear(128, 64)
        self.out = nn.Linear(64, 1)
        for m in self.modules():
            if isinstance(m, (nn.Conv1d, nn.Linear)):
                nn.init.xavier_uniform_(m.weight)
                nn.init.zeros_(m.bias)

    def recurrent_block(self, x):
        raise NotImplementedError

    def forward(self, x):
        """x: [B, T, 12] (channels last, any float dtype) -> raw output [B, 1]"""
        x = x.to(self.conv1.weight.dtype).transpose(1, 2)
        x = F.relu(self.bn1(self.conv1(ConvNet._same(x))))
        x = F.relu(self.bn2(self.conv2(ConvNet._same(x))))
        x = self.conv3(ConvNet._same(x))                    # [B, 256, 25]; no BN / activation on the last conv
        x = self.recurrent_block(x.transpose(1, 2))         # fp64 inside (the layers cast at their door)
        x = x.to(self.fc1.weight.dtype)
        x = F.relu(self.fbn1(self.fc1(x)))
        x = F.relu(self.fbn2(self.fc2(x)))
        x = F.relu(self.fbn3(self.fc3(x)))
        x = self.fc4(x)
        return self.out(x)


class ConvBiLstmNet(_ConvRecurrentNet):
    def __init__(self, in_channels=12, impl="auto"):
        super().__init__(256, in_channels)
        self.lstm = KerasBidirectional(KerasLSTM(256, 128, impl=impl), KerasLSTM(256, 128, go_backwards=True, impl=impl))

    def recurrent_block(self, x):
        return self.lstm(x)


class ConvLstmNet(_ConvRecurrentNet):
    def __init__(self, in_channels=12, impl="auto"):
        super().__init__(128, in_channels)
        self.lstm1 = KerasLSTM(256, 128, return_sequences=True, impl=impl)
        self.lstm2 = KerasLSTM(128, 128, impl=impl)

    def recurrent_block(self, x):
        return self.lstm2(self.lstm1(x))


def make_model(model_type, **kw):
    """training_cross_validate.py's three names: conv, conv_lstm, conv_bilstm; as there, anything else is the ConvNet"""
    if model_type == "conv_lstm":
        return ConvLstmNet(**kw)
    if model_type == "conv_bilstm":
        return ConvBiLstmNet(**kw)
    return ConvNet()
