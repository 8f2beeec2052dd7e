"""NumPy restatement of soft-grip_amd/lstm.py's layer (Keras' LSTM: gate order i, f, c~, o; sigmoid / tanh; zero initial state unless
given), forward and hand-written backward through time -- the independent side of tests/test_lstm_host.py, as np_convnet.py is for
the ConvNet.  Everything in float64; x is taken in TIME order and reversed here for go_backwards."""
import numpy as np


def sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def forward(kernel, recurrent, bias, x, go_backwards=False, h0=None, c0=None):
    """x [B, T, D] -> dict: h_seq, c_seq [B, T, H] and gates [B, T, 4H] (activated), all in consumption order, and xs (x as consumed)"""
    xs = x[:, ::-1] if go_backwards else x
    B, T, _ = xs.shape
    H = recurrent.shape[0]
    h = np.zeros((B, H)) if h0 is None else h0
    c = np.zeros((B, H)) if c0 is None else c0
    hs, cs, gs = np.zeros((B, T, H)), np.zeros((B, T, H)), np.zeros((B, T, 4 * H))
    for t in range(T):
        a = xs[:, t] @ kernel + bias + h @ recurrent
        i, f, g, o = sigmoid(a[:, :H]), sigmoid(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), sigmoid(a[:, 3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
        hs[:, t], cs[:, t], gs[:, t] = h, c, np.concatenate([i, f, g, o], axis=1)
    return dict(h_seq=hs, c_seq=cs, gates=gs, xs=xs)


def backward(kernel, recurrent, fw, dh_seq, go_backwards=False, h0=None, c0=None):
    """fw: forward()'s dict; dh_seq [B, T, H]: the gradient with respect to h_seq (consumption order) -> dict: dz [B, T, 4H]
    (consumption order), dx [B, T, D] (TIME order), dkernel, drecurrent, dbias, dh0, dc0"""
    hs, cs, gs, xs = fw["h_seq"], fw["c_seq"], fw["gates"], fw["xs"]
    B, T, H = hs.shape
    dz = np.zeros((B, T, 4 * H))
    dh_rec, dc = np.zeros((B, H)), np.zeros((B, H))
    for t in range(T - 1, -1, -1):
        i, f, g, o = gs[:, t, :H], gs[:, t, H:2 * H], gs[:, t, 2 * H:3 * H], gs[:, t, 3 * H:]
        c_prev = cs[:, t - 1] if t > 0 else (np.zeros((B, H)) if c0 is None else c0)
        dh = dh_seq[:, t] + dh_rec
        tc = np.tanh(cs[:, t])
        dc = dc + dh * o * (1.0 - tc * tc)
        dz[:, t] = np.concatenate([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], axis=1)
        dc = dc * f
        dh_rec = dz[:, t] @ recurrent.T
    h_prev = np.concatenate([(np.zeros((B, 1, H)) if h0 is None else h0[:, None]), hs[:, :-1]], axis=1)
    dxs = dz @ kernel.T
    return dict(dz=dz, dx=dxs[:, ::-1] if go_backwards else dxs,
                dkernel=np.einsum("btd,btg->dg", xs, dz), drecurrent=np.einsum("bth,btg->hg", h_prev, dz), dbias=dz.sum(axis=(0, 1)),
                dh0=dh_rec, dc0=dc)
