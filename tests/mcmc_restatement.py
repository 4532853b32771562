"""Host-side restatements shared by the slice-sampler tests: the per-chain transitions of the vectorised slice sampler
(slice_numpy.py:438-566) on tensors, Philox4x32-10 in numpy, and the uniforms the device samplers draw from it.

Nothing here imports the library: these are the oracles the kernels are compared with."""

import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)      # Salmon et al., SC'11, table 2
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)      # Weyl increments of the key schedule


def philox4x32_10(counter, key):
    """Philox4x32-10 on arrays: `counter` four and `key` two broadcastable arrays of 32-bit words; four uint64 arrays
    holding 32-bit words come back.  All arithmetic in uint64 (a 32 x 32 product fits)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & M32 for k in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def u01(r):
    """The top 24 bits of a 32-bit word as a float32 in [0, 1): (r >> 8) * 2**-24, exact."""
    return ((np.asarray(r, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0**-24).astype(np.float32)


def tick_uniforms(seed, tick_no, num_chains, dim):
    """(C, 4 + D) float32: what one tick of the device samplers draws when no host uniforms are passed.  Counter
    (tick lo, tick hi, chain, block), key (seed lo, seed hi); block 0 gives u[0..3]; lane d & 3 of block 1 + (d >> 2)
    gives the shuffle uniform of dimension d (column 4 + d)."""
    seed, tick_no = int(seed), int(tick_no)
    chain = np.arange(num_chains, dtype=np.uint64)
    ctr = lambda block: (tick_no & 0xFFFFFFFF, tick_no >> 32, chain, block)      # noqa: E731
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty((num_chains, 4 + dim), dtype=np.float32)
    for q, r in enumerate(philox4x32_10(ctr(0), key)):
        out[:, q] = u01(r)
    for block in range(1, 2 + ((dim - 1) >> 2)):
        words = philox4x32_10(ctr(block), key)
        for lane in range(4):
            d = 4 * (block - 1) + lane
            if d < dim:
                out[:, 4 + d] = u01(words[lane])
    return torch.from_numpy(out)


def torch_tick(st, logp, u, num_samples, tuning, max_width):
    """Tensorised restatement of the per-chain transitions of slice_numpy.py:438-566 (test oracle for the
    tick kernel; consumes the same uniforms).  Every comparison is the reference's: a NaN log-density stops bracket
    growth in LOWER / UPPER (`>=` is false) and is accepted in SAMPLE_SLICE (`<` is false).

    Returns what the tick met, for tests that must prove a branch was taken: `capped`, the LOWER / UPPER visits at
    which log p >= logu held and the width test alone stopped the growth, and `nonfinite`, per state (BEGIN, LOWER,
    UPPER, SAMPLE) the live chains whose log-density was -inf, +inf or NaN."""
    x, nxt, width, order, state, i, t, cxi, wi, lx, ux, xi, logu, samples = (st[k] for k in (
        "x", "nxt", "width", "order", "state", "i", "t", "cxi", "wi", "lx", "ux", "xi", "logu", "samples"))
    C, D = x.shape
    ar = torch.arange(C, device=x.device)
    dim = order[ar, i]
    live = state != 4
    is_b, is_l, is_u, is_s = (live & (state == k) for k in range(4))
    # BEGIN
    cxi = torch.where(is_b, x[ar, dim], cxi)
    wi = torch.where(is_b, width[ar, dim], wi)
    logu = torch.where(is_b, logp + torch.log(1.0 - u[:, 0]), logu)
    lx_b = cxi - wi * u[:, 1]
    # LOWER
    above = logp >= logu
    out_l = is_l & above & (cxi - lx < max_width)
    # UPPER
    out_u = is_u & above & (ux - cxi < max_width)
    capped = int(((is_l & above & ~out_l) | (is_u & above & ~out_u)).sum())
    bad = ~torch.isfinite(logp)
    nonfinite = [int((s & bad).sum()) for s in (is_b, is_l, is_u, is_s)]
    # SAMPLE
    rej = is_s & (logp < logu)
    acc = is_s & ~rej
    new_lx = torch.where(is_b, lx_b, torch.where(out_l, lx - wi, torch.where(rej & (xi < cxi), xi, lx)))
    new_ux = torch.where(is_b, lx_b + wi, torch.where(out_u, ux + wi, torch.where(rej & ~(xi < cxi), xi, ux)))
    draw = (new_ux - new_lx) * u[:, 2] + new_lx
    new_xi = torch.where((is_u & ~out_u) | rej, draw, xi)
    val = torch.where(is_b | out_l, new_lx, torch.where((is_l & ~out_l) | out_u, new_ux, new_xi))
    write = live & ~acc
    nxt[ar[write], dim[write]] = val[write]
    x[ar[acc], dim[acc]] = xi[acc]
    tune = acc & (t < tuning)
    w_old = width[ar[tune], dim[tune]]
    width[ar[tune], dim[tune]] = w_old + ((ux[tune] - lx[tune]) - w_old) / (t[tune] + 1).float()
    sweep_end = acc & (i == D - 1)
    store = sweep_end & (t >= tuning)
    samples[ar[store], (t[store] - tuning)] = x[store]
    # fresh order by Fisher-Yates on the same uniforms (float32 product, as in the kernel)
    rows = ar[sweep_end]
    if rows.numel():
        o = torch.arange(D, device=order.device, dtype=order.dtype).repeat(rows.numel(), 1)
        r = torch.arange(rows.numel(), device=order.device)
        for d in range(D - 1, 0, -1):
            k = (u[rows, 4 + d] * torch.tensor(float(d + 1), dtype=torch.float32, device=u.device)).long().clamp(max=d)
            od, ok = o[:, d].clone(), o[r, k].clone()
            o[:, d] = ok
            o[r, k] = od
        order[rows] = o
    new_state = torch.where(is_b, 1, torch.where(is_l & ~out_l, 2, torch.where(is_u & ~out_u, 3,
                            torch.where(acc, 0, state))))
    t = torch.where(sweep_end, t + 1, t)
    i = torch.where(acc, torch.where(sweep_end, torch.zeros_like(i), i + 1), i)
    new_state = torch.where(sweep_end & (t >= num_samples + tuning), 4, new_state)
    st.update(state=new_state, i=i, t=t, cxi=cxi, wi=wi, lx=new_lx, ux=new_ux, xi=new_xi, logu=logu)
    return dict(capped=capped, nonfinite=nonfinite)


def restatement_state(x0, order0, width0, num_samples):
    """The restatement's state for chains starting at `x0` with dimension order `order0` and bracket widths `width0`."""
    C, D = x0.shape
    dev = x0.device
    return dict(x=x0.clone(), nxt=x0.clone(), width=torch.full((C, D), float(width0), device=dev),
                order=order0.clone().long(), state=torch.zeros(C, dtype=torch.long, device=dev),
                i=torch.zeros(C, dtype=torch.long, device=dev), t=torch.zeros(C, dtype=torch.long, device=dev),
                samples=torch.zeros(C, num_samples, D, device=dev),
                **{k: torch.zeros(C, device=dev) for k in ("cxi", "wi", "lx", "ux", "xi", "logu")})


def kernel_state(x0, order0, width0, num_samples):
    """The buffers of sbi_amd_mcmc_slice_tick for the same start."""
    C, D = x0.shape
    dev = x0.device
    return dict(x=x0.clone(), nxt=x0.clone(), width=torch.full((C, D), float(width0), device=dev),
                order=order0.clone().to(torch.int32).contiguous(), istate=torch.zeros(C, 4, dtype=torch.int32, device=dev),
                fstate=torch.zeros(C, 8, device=dev), samples=torch.zeros(C, num_samples, D, device=dev),
                done=torch.zeros(1, dtype=torch.int32, device=dev))
