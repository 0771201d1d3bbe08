"""Which native op the fused nodes call, on which stream, with which sink and which accumulator (GPU).

One forward + backward of a whole model per configuration (``scripts/dump_block_calls.py`` CONFIGS:
ResNet-50 / ResNet-18 on batch 8 of 64 px images, in a DDP flat space or not, default /
deterministic / fp8 / without the atomic BN sums / eval) is recorded call by call -- op, stream role,
and for every argument and result its dtype, shape and alias id -- and compared per autograd node
with tests/golden/block_calls.json, which holds the line count and sha256 of each node's lines as
recorded before ``ops/fused.py`` was rebuilt around unit records.  A restructure of that file must
leave every line as it was.  On a mismatch the first differing node's lines are printed; diff them
against ``scripts/dump_block_calls.py --text DIR`` of the commit that wrote the golden.

After the step every persistent accumulator (``_pdt_bacc``, ``_pdt_facc``, ``_pdt_csum`` of each
parameter, every ``_FOLD_WS`` workspace) must be all zero again, and FOLD_CALLS / DUAL_CALLS must
have advanced by the recorded counts.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump_module():
    spec = importlib.util.spec_from_file_location(
        "dump_block_calls", os.path.join(ROOT, "scripts", "dump_block_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dump = _dump_module()


@pytest.fixture(scope="module")
def golden():
    with open(dump.GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_configuration(golden):
    assert sorted(golden) == sorted(dump.CONFIGS)
    assert len(dump.CONFIGS) == 8


@pytest.mark.parametrize("name", list(dump.CONFIGS))
def test_block_calls_match_golden(gpu, golden, name):
    res = dump.run_config(name, gpu)
    want = golden[name]
    got = json.loads(json.dumps(dump.digest(res)))
    for i, (w, g) in enumerate(zip(want["nodes"], got["nodes"])):
        if w != g:
            print(f"{name}: first differing node {g[0]!r} (golden {w[0]!r}, {w[1]} lines; now {g[1]} lines):")
            print("\n".join(res["sections"][i][1]))
            break
    assert got["nodes"] == want["nodes"]
    assert (got["fold_calls"], got["dual_calls"]) == (want["fold_calls"], want["dual_calls"])
    assert not res["nonzero"], res["nonzero"]
