"""The launch policy of the implicit-GEMM convolutions, pinned against tests/golden/nt_plan.json
(written by scripts/dump_nt_plan.py): which NT tile and BN row group every forward GEMM and every
input-gradient parity class of ResNet-18 / ResNet-50 gets at three (batch, resolution) points, at
bf16 and at fp8 operand bytes, their weight-gradient plans, and the NT tile over a grid of
(M, Nout, B-row bytes) that straddles every constant of the policy, with and without the
``conv_nt_force`` overrides.  Fails when a change to the plan functions moves any launch.

The plan functions run on the host, so this needs no GPU.  The weight-gradient plans depend on the
CU count: without a device ``wg_cus()`` falls back to 256, which is also the MI355X's count, so the
golden is the same with and without the GPU."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump_module():
    spec = importlib.util.spec_from_file_location("dump_nt_plan", os.path.join(ROOT, "scripts", "dump_nt_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_nt_plan_matches_golden(native_ext):
    dump = _dump_module()
    with open(dump.GOLDEN) as f:
        want = json.load(f)
    try:
        got = json.loads(json.dumps(dump.collect(native_ext)))  # tuples as JSON spells them
    finally:
        native_ext.conv_nt_force(-1, -1, -1)
    # the golden covers what it should: the 20 and 53 convolutions (stem included) at three points each,
    # and 648 grid points per override
    assert len(want["resnet"]) == 3 * (20 + 53)
    assert sorted(want["grid"]) == ["mid_off", "policy", "wide_off"]
    assert all(len(rows) == 8 * 9 * 9 for rows in want["grid"].values())
    assert len(got["resnet"]) == len(want["resnet"])
    for g, w in zip(got["resnet"], want["resnet"]):
        assert g == w, (w["model"], w["batch"], w["res"], w["name"])
    assert got["grid_columns"] == want["grid_columns"]
    for key, rows in want["grid"].items():
        assert len(got["grid"][key]) == len(rows)
        for g, w in zip(got["grid"][key], rows):
            assert g == w, (key, w)
