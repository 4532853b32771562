"""fp64 restatement of SpectralConvEmbedding and of its parameter gradient, written from the published formula with real
cosine / sine matrices and an explicit backward pass (no complex tensors, no autograd): the reference of the kernel parity
tests.  tests/test_sc_embedding_cpu.py ties it to the recording of the real sbi class.

theta[b, k, n] = 2 pi k t[b, n], t the fp32 position promoted to fp64, or n / n_points exactly on the equispaced grid.
  h_0 = fc0(x);   (A, B)[k, i] = (1 / N) sum_n (cos, -sin) theta h_l[n, i]              the coefficients Re, Im
  (P, Q)[k, o] = sum_i (A Wr - B Wi, A Wi + B Wr)[i, o, k]                               the per-mode complex mix
  u_l[n, o] = sum_k cos theta P - sin theta Q + sum_i w[o, i] h_l[n, i] + b[o];   h_{l+1} = gelu(u_l), exact erf
  out[(2 k + r) out_channels + o] = fc_last.bias[o] + sum_c fc_last.weight[o, c] (r ? Q : P)_last[k, c]
The gradient is flat in state_dict order; a complex weight's is (dL/dRe, dL/dIm) pairs, torch's convention."""
import math

import torch


def _phases(x, modes):
    """(values (B, N, Cin), cos, sin (B, M, N)) in fp64"""
    x = x.detach().cpu()
    if x.ndim == 4:
        values, t = x[:, 0].double(), x[:, 1, 0, :].double()
    else:
        n = x.shape[-1]
        values, t = x.double(), (torch.arange(n, dtype=torch.float64) / n).expand(x.shape[0], n)
    theta = 2 * math.pi * torch.arange(modes, dtype=torch.float64)[None, :, None] * t[:, None, :]
    return values.permute(0, 2, 1), torch.cos(theta), torch.sin(theta)


def _parts(w):
    w = w.detach().cpu()
    return w.real.double(), w.imag.double()


def _gelu(u):
    return 0.5 * u * (1 + torch.erf(u / math.sqrt(2)))


def _dgelu(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def reference(state_dict, x, wts):
    """(out (B, 2 modes out_channels), flat gradient of sum(wts * out)) in fp64 from the fp32 state_dict and input"""
    sd = state_dict
    L = sum(1 for k in sd if k.startswith("conv_layers."))
    modes = sd["conv_last.weights1"].shape[-1]
    values, cs, sn = _phases(x, modes)
    B, N, _ = values.shape
    f = lambda k: sd[k].detach().cpu().double()      # noqa: E731
    spectral = [_parts(sd[f"conv_layers.{l}.weights1"]) for l in range(L)] + [_parts(sd["conv_last.weights1"])]

    def coefficients(h):
        return torch.einsum("bkn,bni->bki", cs, h) / N, -torch.einsum("bkn,bni->bki", sn, h) / N

    def mix(a, b, wr, wi):
        return (torch.einsum("bki,iok->bko", a, wr) - torch.einsum("bki,iok->bko", b, wi),
                torch.einsum("bki,iok->bko", a, wi) + torch.einsum("bki,iok->bko", b, wr))

    hs, us, coeffs = [values @ f("fc0.weight").T + f("fc0.bias")], [], []
    for l in range(L):
        a, b = coefficients(hs[-1])
        p, q = mix(a, b, *spectral[l])
        w = f(f"w_layers.{l}.weight")[..., 0]
        u = (torch.einsum("bkn,bko->bno", cs, p) - torch.einsum("bkn,bko->bno", sn, q) + hs[-1] @ w.T
             + f(f"w_layers.{l}.bias"))
        coeffs.append((a, b))
        us.append(u)
        hs.append(_gelu(u))
    a, b = coefficients(hs[-1])
    coeffs.append((a, b))
    p, q = mix(a, b, *spectral[L])
    z = torch.stack([p, q], dim=2).reshape(B, 2 * modes, -1)                   # row 2 k + r
    flw = f("fc_last.weight")
    out = (z @ flw.T + f("fc_last.bias")).reshape(B, -1)

    # ---- backward ----
    g = wts.detach().cpu().double().reshape(B, 2 * modes, -1)
    grads = {"fc_last.weight": torch.einsum("bro,brc->oc", g, z), "fc_last.bias": g.sum(dim=(0, 1))}
    gz = (g @ flw).reshape(B, modes, 2, -1)
    gp, gq = gz[:, :, 0], gz[:, :, 1]

    def mix_backward(a, b, wr, wi, gp, gq):
        """(dL/dWr, dL/dWi, dL/da, dL/db)"""
        return (torch.einsum("bki,bko->iok", a, gp) + torch.einsum("bki,bko->iok", b, gq),
                torch.einsum("bki,bko->iok", a, gq) - torch.einsum("bki,bko->iok", b, gp),
                torch.einsum("bko,iok->bki", gp, wr) + torch.einsum("bko,iok->bki", gq, wi),
                torch.einsum("bko,iok->bki", gq, wr) - torch.einsum("bko,iok->bki", gp, wi))

    def coefficients_backward(ga, gb):
        return (torch.einsum("bkn,bki->bni", cs, ga) - torch.einsum("bkn,bki->bni", sn, gb)) / N

    dwr, dwi, ga, gb = mix_backward(*coeffs[L], *spectral[L], gp, gq)
    grads["conv_last.weights1"] = torch.stack([dwr, dwi], dim=-1)
    gh = coefficients_backward(ga, gb)
    for l in range(L - 1, -1, -1):
        gu = gh * _dgelu(us[l])
        w = f(f"w_layers.{l}.weight")[..., 0]
        grads[f"w_layers.{l}.weight"] = torch.einsum("bno,bni->oi", gu, hs[l])
        grads[f"w_layers.{l}.bias"] = gu.sum(dim=(0, 1))
        gp, gq = torch.einsum("bkn,bno->bko", cs, gu), -torch.einsum("bkn,bno->bko", sn, gu)
        dwr, dwi, ga, gb = mix_backward(*coeffs[l], *spectral[l], gp, gq)
        grads[f"conv_layers.{l}.weights1"] = torch.stack([dwr, dwi], dim=-1)
        gh = gu @ w + coefficients_backward(ga, gb)
    grads["fc0.weight"] = torch.einsum("bnc,bni->ci", gh, values)
    grads["fc0.bias"] = gh.sum(dim=(0, 1))
    return out, torch.cat([grads[k].reshape(-1) for k in sd])


def flat_grad(net):
    """the flat gradient of a module after backward, complex entries as (re, im) pairs"""
    return torch.cat([(torch.view_as_real(p.grad) if p.is_complex() else p.grad).reshape(-1)
                      for p in net.parameters()])


def golden_net(cls, case):
    """the module of a recorded case (tools/make_golden_sc_embedding.py) with the recorded weights"""
    net = cls(**case["kwargs"])
    net.load_state_dict(case["state_dict"], strict=True)
    return net
