"""GPU: stream order and graph replay of the model handles (`stream_cases.py`).

Every test of `test_guard_model_gpu.py` - `frmap_model_forward` of every family and selector, fp32 and uint8 input, the three stems,
both batch sizes; `frmap_model_embed_and_match` / `_embed_and_search` with scanned and packed galleries, with and without the
normalise step - runs again under the late rule and under the capture rule.  The handles are built outside the closures, so only
`x` and the gallery operands are placed (late, or static buffers of the graph); `match_prepare` runs inside the closure: the pack is
built on the late stream, or inside the graph, and `wait_ready` is recorded and waited for there.
"""
import pytest

pytestmark = pytest.mark.gpu

import stream_cases as sc  # noqa: E402
import test_guard_model_gpu as tm  # noqa: E402

MIRRORED = ["test_resnet_handle_forward", "test_resnet_handle_forward_bf16", "test_family_handle_forward",
            "test_siamese_u8_unfused_stem", "test_embed_and_match_and_search"]
assert set(MIRRORED) == {n for n in dir(tm) if n.startswith("test_")}

for _name in MIRRORED:
    assert sc.CAPTURABLE[_name] is True
    globals()[_name + "_late"] = sc.mirror_late(tm, _name)
    globals()[_name + "_captured"] = sc.mirror_capture(tm, _name)


def test_stream_report(capsys):
    assert sc.CALLS["late"] > 0 and sc.CALLS["capture"] > 0
    with capsys.disabled():
        print("\n[test_stream_model_gpu] " + sc.report(MIRRORED))
