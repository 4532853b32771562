"""Host-only table of the NSF routing and workspace decisions: which kernel family and image an n-row call takes, and
how large / where the training workspace and its parts are.  No GPU needed.

Run it against two builds of the library and diff the output to show that a host-side change moved no decision:

    SBI_AMD_LIB=path/to/libsbi_amd_nsf.so python tools/route_table.py > before.json
"""
import ctypes
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from sbi_amd import _lib  # noqa: E402
from sbi_amd.neural_nets.estimators.nsf_flow import NSFHyper  # noqa: E402

CONFIGS = {
    "default": dict(),
    **{f"K{k}": dict(num_bins=k) for k in (4, 5, 8, 16)},
    "hidden100": dict(hidden_features=100),                   # wide cooperative kernels
    "D20": dict(D=20),                                        # generic training pass
    "blocks3": dict(num_blocks=3),                            # generic training pass
    "ctx_layers2": dict(D=1, hidden_layers_spline_context=2),
    "ctx_layers_none": dict(D=1, hidden_layers_spline_context=0),
}
ROWS = (1, 200, 8192, 8193, 12288, 12289, 65536, 10**6)
BASE = 1 << 20          # a dummy workspace address: sqnorm_parts is reported as an offset from it (bytes / 4)


def rows_of(lib, c):
    out = {}
    for n in ROWS:
        parts = ctypes.c_int64(-1)
        p = lib.sbi_amd_nsf_train_sqnorm_parts(c, n, BASE, ctypes.byref(parts))
        out[n] = dict(ws=lib.sbi_amd_nsf_train_workspace_floats(c, n),
                      sq_off=None if not p else (p - BASE) // 4, sq_parts=parts.value,
                      kind_eval=lib.sbi_amd_nsf_image_kind(c, n, 0), kind_train=lib.sbi_amd_nsf_image_kind(c, n, 1),
                      waves_eval=lib.sbi_amd_nsf_plan_waves(c, n, 0), waves_sample=lib.sbi_amd_nsf_plan_waves(c, n, 1))
    return out


def main():
    lib = _lib.load(build_if_missing=False)
    table = {}
    for threshold in ("default", "coop_off"):
        if threshold == "coop_off":
            lib.sbi_amd_nsf_set_coop_max_rows(0)
        for name, kw in CONFIGS.items():
            c = NSFHyper(**{**dict(D=10, C=10), **kw}).c_config()
            table[f"{threshold}/{name}"] = dict(packed=lib.sbi_amd_nsf_packed_floats(c),
                                                step_map_ws=lib.sbi_amd_nsf_step_map_workspace_floats(c),
                                                rows=rows_of(lib, c))
    json.dump(table, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
