"""real_amd/csrc/real_hip_internal.h holds the device views and nothing of the host layer.

bench.kernel_source_hash() hashes that file to tie profiles/traffic.json to the matcher it was measured on, so what kernels
do not read stays out of it: the host context (real_hip_ctx.h), the owned buffers and the stage records (host_buf.h,
<stage>_stage.h).  The headers that only kernels use include the device views alone.
"""
import os
import re


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "real_amd", "csrc")
KERNEL_ONLY = ("kernel_common.h", "match_common.h", "read_words.h", "row_bytes.h", "complex_walk.h")


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def test_internal_header_holds_no_host_layer():
    text = _text("real_hip_internal.h")
    for word in ("struct real_hip_ctx {", "DevBuf", "RhStage", "hipStream_t", "hipEvent_t"):
        assert word not in text, word
    includes = re.findall(r'#include\s+"([^"]+)"', text)
    assert sorted(includes) == ["index_plan.h", "real_hip.h", "row_addr.h"], includes
    for view in ("struct DevText {", "struct DevIndex {", "struct DevBatch {", "struct MatchArgs {"):
        assert view in text, view


def test_kernel_only_headers_do_not_include_the_host_layer():
    host = {"real_hip_ctx.h", "host_buf.h"} | {n for n in os.listdir(CSRC) if n.endswith("_stage.h")}
    seen = set()

    def closure(name):  # every project header `name` includes, directly or not
        if name in seen or not os.path.exists(os.path.join(CSRC, name)):
            return
        seen.add(name)
        for inc in re.findall(r'#include\s+"([^"]+)"', _text(name)):
            closure(inc)

    for name in KERNEL_ONLY:
        closure(name)
    assert set(KERNEL_ONLY) <= seen and "real_hip_internal.h" in seen
    assert not (seen & host), sorted(seen & host)


def test_every_stage_record_is_a_member_of_the_context():
    ctx = _text("real_hip_ctx.h")
    stage_headers = sorted(n for n in os.listdir(CSRC) if n.endswith("_stage.h"))
    assert len(stage_headers) == 14, stage_headers
    for name in stage_headers:
        assert '#include "%s"' % name in ctx, name
        records = re.findall(r"^struct (Rh\w+Stage) \{", _text(name), re.M)
        assert len(records) == 1, (name, records)
        assert re.search(r"^    %s \w+;" % records[0], ctx, re.M), records[0]
