"""The Python surface of the native extension: every public name of `_C`, its parameter names, order
and defaults, and the members of its three classes, against tests/golden/c_api.json (written by
scripts/dump_c_api.py from the single-file bindings before they were split by op family).  Fails when
a binding source drops an op, renames an argument or loses a default.  Needs no GPU."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump_module():
    spec = importlib.util.spec_from_file_location("dump_c_api", os.path.join(ROOT, "scripts", "dump_c_api.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_c_api_matches_golden(native_ext):
    dump = _dump_module()
    with open(dump.GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(dump.describe(native_ext)))  # tuples / None as JSON spells them
    classes = sorted(k for k, v in want.items() if isinstance(v, dict))
    assert len(want) == 78 and classes == ["RcclComm", "Reducer", "XgmiComm"]
    assert sorted(got) == sorted(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    for name in sorted(want):
        assert got[name] == want[name], name
    # the signature lines parse: an op with keyword arguments shows them, with defaults
    assert want["conv_wgrad"][0][-2:] == [["deterministic", "False"], ["out", "None"]]
    assert all(sigs for sigs in want.values())
