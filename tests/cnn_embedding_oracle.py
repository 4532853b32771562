"""fp64 restatement of CNNEmbedding's convolution stack (sbi/neural_nets/embedding_nets/cnn.py) with explicit index
arithmetic: gather the patches of the zero-padded map, multiply by the weights, sum; ReLU; gather the pool windows,
take the maximum.  No conv / pool library call.  Gradients come by autograd in fp64 on that formula.  Weights are a
list [W0, b0, W1, b1, ...] in state_dict order; a 1-D stack is the 2-D one with a single unpadded row.

Separation.  For every conv pre-activation u let S = sum |w x| + |b|: an f32 fma chain stays within about 1.5e-7 S of
fp64.  A case is well separated when every |u| >= 32 * 2^-24 * S and, in every pool window whose maximum is positive,
the top two values differ by at least 32 * 2^-24 times the larger S of the two.  Below that margin a rounding flips a
ReLU mask or an argmax and the gradient changes by an O(1) amount, in the kernel and in eager torch alike.
`separation` is the smallest of these margins in units of 32 * 2^-24 S: >= 1 means well separated."""
import torch

MARGIN = 32 * 2.0**-24


def _as_2d(x, params):
    """(x (B, C, H, W), [(W (O, C, KH, k), b)], pad_y, 1-D?)"""
    one = params[0].dim() == 3
    if one:
        x = x.unsqueeze(2)
    layers = [(w.unsqueeze(2) if one else w, b) for w, b in zip(params[0::2], params[1::2])]
    return x, layers, (0 if one else 1), one


def _patches(x, KH, k, pad_y):
    """(B, C, KH * k, HC, WC): tap (ky, kx) of output (oy, ox) is the padded map at (oy + ky, ox + kx)."""
    B, C, H, W = x.shape
    xp = x.new_zeros(B, C, H + 2 * pad_y, W + 2)
    xp[:, :, pad_y:pad_y + H, 1:1 + W] = x
    HC, WC = H + 2 * pad_y - KH + 1, W + 3 - k
    return torch.stack([xp[:, :, ky:ky + HC, kx:kx + WC] for ky in range(KH) for kx in range(k)], dim=2)


def _windows(u, PH, PW):
    """(B, O, HP, WP, PH * PW) in row-major window order; trailing rows / columns that fill no window are dropped."""
    B, O, HC, WC = u.shape
    HP, WP = HC // PH, WC // PW
    u = u[:, :, :HP * PH, :WP * PW].reshape(B, O, HP, PH, WP, PW)
    return u.permute(0, 1, 2, 4, 3, 5).reshape(B, O, HP, WP, PH * PW)


def cnn_forward(params, x, pool_kernel_size, report=None):
    """x (B, C, spatial...) -> features (B, F), channel-major.  `report`: a list that receives the separation."""
    h, layers, pad_y, one = _as_2d(x, params)
    PW = int(pool_kernel_size)
    PH = 1 if one else PW
    sep = float("inf")
    for w, b in layers:
        O, C, KH, k = w.shape
        pt = _patches(h, KH, k, pad_y)                                        # (B, C, T, HC, WC)
        wt = w.reshape(O, C, KH * k)
        u = (pt.unsqueeze(1) * wt[None, :, :, :, None, None]).sum(dim=(2, 3)) + b[None, :, None, None]
        r = torch.clamp(u, min=0.0)
        win = _windows(r, PH, PW)
        if report is not None:
            with torch.no_grad():
                S = (pt.abs().unsqueeze(1) * wt.abs()[None, :, :, :, None, None]).sum(dim=(2, 3))
                S = S + b.abs()[None, :, None, None]
                sep = min(sep, (u.abs() / (MARGIN * S)).min().item())
                top, idx = win.topk(2, dim=-1)
                s2 = _windows(S, PH, PW).gather(-1, idx).amax(dim=-1)
                gap = (top[..., 0] - top[..., 1]) / (MARGIN * s2)
                live = top[..., 0] > 0
                if live.any():
                    sep = min(sep, gap[live].min().item())
        h = win.max(dim=-1).values
    if report is not None:
        report.append(sep)
    return h.reshape(h.shape[0], -1)


def to64(params):
    return [p.detach().double().cpu().clone().requires_grad_(True) for p in params]


def cnn_reference(params, x, wts, pool_kernel_size, want_dx=False):
    """(features, flat parameter gradient, separation, dx | None) of sum(features * wts) in fp64."""
    p64 = to64(params)
    x64 = x.detach().double().cpu().clone().requires_grad_(want_dx)
    report = []
    out = cnn_forward(p64, x64, pool_kernel_size, report)
    grads = torch.autograd.grad((out * wts.double().cpu()).sum(), p64 + ([x64] if want_dx else []))
    flat = torch.cat([g.reshape(-1) for g in grads[:len(p64)]])
    return out.detach(), flat, report[0], (grads[-1] if want_dx else None)


def sizes(spatial, out_channels, kernel_size, pool_kernel_size):
    """[(input extents, conv extents, pool extents)] per layer as (H, W) pairs (H = 1 in 1-D), or None when the map
    shrinks to 0."""
    two = len(spatial) == 2
    H, W = (spatial if two else (1, spatial[0]))
    out = []
    for _ in out_channels:
        HC, WC = (H + 3 - kernel_size if two else 1), W + 3 - kernel_size
        if HC < 1 or WC < 1:
            return None
        HP, WP = (HC // pool_kernel_size if two else 1), WC // pool_kernel_size
        if HP < 1 or WP < 1:
            return None
        out.append(((H, W), (HC, WC), (HP, WP)))
        H, W = HP, WP
    return out


def lds_bytes(spatial, in_channels, out_channels, kernel_size, pool_kernel_size):
    """the documented backward image (include/sbi_amd_cnn.h): weights and their accumulators, every layer's
    zero-bordered input map with an odd row stride, the pool selections, the gated gradient, the dense conv gradient"""
    two = len(spatial) == 2
    chans = [in_channels] + list(out_channels)
    taps = kernel_size**2 if two else kernel_size
    P = sum(chans[i + 1] * chans[i] * taps + chans[i + 1] for i in range(len(out_channels)))
    maps = sel = gmax = dmax = 0
    for i, ((H, W), (HC, WC), (HP, WP)) in enumerate(sizes(spatial, out_channels, kernel_size, pool_kernel_size)):
        maps += chans[i] * (H + 2 if two else 1) * ((W + 2) | 1)
        sel += chans[i + 1] * HP * WP
        gmax = max(gmax, chans[i + 1] * HP * WP)
        if i >= 1:
            dmax = max(dmax, chans[i + 1] * HC * WC)
    return 4 * (2 * P + maps + sel + gmax + dmax)
