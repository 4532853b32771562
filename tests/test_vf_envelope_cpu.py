"""The case table of tests/vf_envelope.py against the host plan (csrc/fmpe_kernel.h::fm_build_plan through the C ABI)
and against a restatement of the kernels' dispatch rules.  Guards the table, not the kernels: every case must be
accepted, and together the cases must reach every HB instantiation, every (OT, KT) weight-gradient instantiation and
both parities of the staging-group count."""

from tests.vf_envelope import (CUS_PLUS_ONE_RAGGED, NET_CASES, SIZE_CASES, dw_pairs_of, hb_of, hyper_of, linears_of,
                               staging_groups)

ROWS = [1, 17, 127, 128, 129, 200, 333, 1025, 2944, 4200, 128 * 256 + 77, 128 * (2 * 256 + 2) + 5]


def test_every_case_is_accepted_by_the_host_plan():
    from sbi_amd import _lib

    lib = _lib.load()
    for cfg in NET_CASES + [c for c, _ in SIZE_CASES] + [dict(D=2, C=4, H=48, L=2, E=32)]:
        h = hyper_of(cfg)
        c = h.c_config()
        assert lib.sbi_amd_fmpe_param_count(c) == h.param_count(), cfg
        assert lib.sbi_amd_fmpe_packed_floats(c) >= 0, cfg
        for n in ROWS:
            assert lib.sbi_amd_fmpe_train_workspace_floats(c, n) >= 0, (cfg, n)


def test_the_table_reaches_every_instantiation():
    assert {hb_of(c) for c in NET_CASES} == {4, 7, 8}
    pairs = {p for c in NET_CASES for p in dw_pairs_of(c)}
    assert pairs == {(o, k) for o in (4, 7, 8) for k in (4, 7, 8)}
    # the two instantiations with PF == false besides 8 x 8, from both sides
    by_case = {(c["D"], c["C"], c["H"]): dict(zip([n for n, _, _ in linears_of(c)], dw_pairs_of(c))) for c in NET_CASES}
    assert by_case[(120, 5, 100)]["IN"] == (7, 8) and by_case[(120, 5, 100)]["OUT"] == (8, 7)
    assert by_case[(70, 6, 128)]["IN"] == (8, 7) and by_case[(70, 6, 128)]["OUT"] == (7, 8)
    assert by_case[(5, 120, 100)]["CT"] == (7, 8)
    # time-embedding blocks: one frequency, a ragged third block, the widest
    assert {(c["E"] + 15) // 16 for c in NET_CASES} == {1, 2, 3, 4}
    assert {c["L"] for c in NET_CASES} >= {1, 2, 7, 8}


def test_the_two_staging_parity_cases_have_six_and_seven_groups():
    ragged = [c for c, n in SIZE_CASES if n == CUS_PLUS_ONE_RAGGED]
    assert [staging_groups(c)[:2] for c in ragged] == [(6, 6), (7, 7)]
    # the restatement of the grouping rule agrees with the plan where the C ABI shows it: the packed image is the
    # groups' images, each padded to 256 floats, so another grouping gives another total
    from sbi_amd import _lib

    lib = _lib.load()
    for cfg in NET_CASES + ragged:
        assert lib.sbi_amd_fmpe_packed_floats(hyper_of(cfg).c_config()) == staging_groups(cfg)[2], cfg
