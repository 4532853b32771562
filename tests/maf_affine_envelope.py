"""Configurations and the host plan of the affine MAF envelope tests (tests/test_maf_affine_envelope_cpu.py and
test_maf_affine_envelope_gpu.py): a restatement in Python of the LDS arithmetic of csrc/maf_affine.hip
(`aff_build_plan`, `aff_plan_for_rows`), written from the layout rules and not from the query's answers, and the
configurations whose workgroup widths the GPU tests claim.  Importable without a GPU; no test functions here.

A config is (D, C, H, NB, T): input features, condition features, hidden features, feed-forward blocks, transforms.
"""

E_UNSUPPORTED, E_BADARG, E_LDS = -1, -2, -3
LDS_LIMIT_BYTES = 160 * 1024
HIDDEN_MAX = 64            # four 16-row hidden tiles
MAX_T, MAX_NB = 16, 4
TRIAL_BLOCK = 8            # MAF_AFF_TC: trials whose flow states a wave keeps in LDS at once
ONE_WAVE_ROWS = 8160       # 510 x 16: the largest launch the halving loop leaves at one wave per workgroup

SMALL = (5, 3, 32, 1, 2)           # KSH 16, ragged everywhere
DEFAULTS = (10, 10, 50, 2, 2)      # sbi's defaults (T = 2 here): KSH 13
CORNER = (16, 32, 64, 4, 2)        # every maximum: the largest LDS footprint
NO_BLOCKS = (5, 3, 32, 0, 2)
TRIALS_SMALL = (3, 4, 24, 2, 3)    # the estimator q(x | theta) of tests/test_maf_affine_gpu.py's trials test

# (config, rows, waves per workgroup): the paired kernels (log_prob, sample, training pass)
WIDE = [(SMALL, 8161, 2), (SMALL, 16321, 4), (SMALL, 32641, 8), (DEFAULTS, 32641, 8), (CORNER, 32641, 8),
        (NO_BLOCKS, 32641, 8)]
# (config, thetas, waves per workgroup): the trials kernel; the second group are the widths its larger scratch (the
# flow states of a block of 8 trials) forces through the 160 KiB limit at 32641 thetas
TRIALS_WIDE = [(TRIALS_SMALL, 8161, 2), (TRIALS_SMALL, 16321, 4), (TRIALS_SMALL, 32641, 8)]
TRIALS_FORCED = [((16, 32, 64, 4, 2), 32641, 4), ((14, 10, 64, 4, 2), 32641, 5), ((8, 32, 64, 4, 2), 32641, 6),
                 ((4, 32, 64, 4, 2), 32641, 7)]


def cfg_id(cfg):
    return "D{}-C{}-H{}-NB{}-T{}".format(*cfg)


# ---------------------------------------------------------------------- the plan of csrc/maf_affine.hip, restated
def _round_up(v, m):
    return (v + m - 1) // m * m


def _two_odd(v):
    """Smallest 2 * odd >= v: row strides that spread the 64 LDS banks."""
    x = (v + 1) // 2
    if x % 2 == 0:
        x += 1
    return 2 * x


def ksh(H):
    """K-steps of the hidden GEMMs: 13 for H in 49..52, else 16."""
    return 13 if (H + 3) // 4 == 13 else 16


def _linear_floats(out, fan_in, bias_pad, ksteps_fixed, min_rows):
    """One linear of the image: rows x ldk weights (at least out + 1 rows: one zero row) and the padded bias."""
    if ksteps_fixed:
        ldk = _two_odd(fan_in)
    else:
        ldk = _two_odd(4 * _round_up((fan_in + 3) // 4, 4))
    return max(out + 1, min_rows) * ldk + bias_pad


def image_floats(D, C, H, NB):
    """Floats of one transform's weight image: initial, context and block linears (each with the 4 KSH + 1 rows the
    transposed GEMMs walk), the two-tile final layer on a 4-float boundary, 8 floats of slack, both permutations."""
    K = ksh(H)
    rows = 4 * K + 1
    l = _linear_floats(H, D, HIDDEN_MAX, 0, rows) + _linear_floats(H, C, HIDDEN_MAX, 0, rows)
    l += NB * _linear_floats(H, H, HIDDEN_MAX, K, rows)
    l = _round_up(l, 4)
    l += _linear_floats(32, H, 32, K, 0)
    l = _round_up(l + 8, 4)
    return _round_up(l + 16 + 16, 4)


def scratch_floats(D, C, trials):
    """Per-wave scratch: the state rows and their copy (16 x ZW + 16 each), the conditioner input rows [z ; context]
    (16 x CINW + 16); the trials kernel adds 8 flow states and 8 x 64 log-det accumulators."""
    ZW = _two_odd(D)
    ks0, ksc = _round_up((D + 3) // 4, 4), _round_up((C + 3) // 4, 4)
    CINW = _two_odd(max(4 * ks0, D + 4 * ksc))
    o = 2 * (16 * ZW + 16) + 16 * CINW + 16
    if trials:
        o += TRIAL_BLOCK * (16 * ZW + 16) + TRIAL_BLOCK * 64
    return _round_up(o, 4)


def lds_bytes(cfg, nw, trials=False):
    D, C, H, NB, _ = cfg
    return 4 * (image_floats(D, C, H, NB) + nw * scratch_floats(D, C, trials))


def refusal(cfg, epsilon=1e-3):
    """The code the plan answers before any arithmetic, or 0."""
    D, C, H, NB, T = cfg
    if D < 1 or C < 1 or H < 1 or T < 1 or NB < 0:
        return E_BADARG
    if D > 16 or C > 32 or H > HIDDEN_MAX or T > MAX_T or NB > MAX_NB:
        return E_UNSUPPORTED
    if not epsilon >= 0.0:
        return E_BADARG
    return 0


def waves(cfg, n, trials=False, epsilon=1e-3):
    """Waves per workgroup of an n-row launch: 8, halved while the rows make fewer than 256 workgroups, then one fewer
    at a time until image + scratch fit the limit; E_LDS when one wave does not."""
    if n < 1:
        return E_BADARG
    rc = refusal(cfg, epsilon)
    if rc:
        return rc
    nw = 8
    while nw > 1 and (n + 16 * nw - 1) // (16 * nw) < 256:
        nw >>= 1
    while nw >= 1:
        if lds_bytes(cfg, nw, trials) <= LDS_LIMIT_BYTES:
            return nw
        nw -= 1
    return E_LDS
