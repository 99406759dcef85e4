"""The kernels whose global-load pipelines wait with hand-counted, non-zero `s_waitcnt vmcnt(n)` assume that the compiler issues
no memory operation of its own inside the pipelined loop.  A register spill would: scratch accesses count in vmcnt, so a count
would become too large and a tile would be read before it has landed.  Checked on the built library's gfx950 code objects:
no private segment, no VGPR or SGPR spill.  CPU only (reads the code-object metadata)."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("SDFA_HIP_LIB") or os.path.join(ROOT, "sdfa-2019_amd", "sdfa_amd", "libsdfa_hip.so")
LLVM = "/opt/rocm/llvm/bin"

# demangled name (a template name stands for every instantiation) -> where its counted waits are
COUNTED_WAITS = {
    "attn_key_score_kernel<1>": "attn.hip, bf16 key/score pass (vmcnt 9..11)",
    "attn_key_score_kernel<3>": "attn.hip, split-bf16 key/score pass (vmcnt 9..11)",
    "attn_key_score_f32_kernel": "attn.hip, fp32 key/score pass (vmcnt 12..16)",
    "attn_fused_f32_kernel": "attn.hip, one-launch fp32 attention layer (vmcnt 4)",
    "freq_lstm_v2_kernel": "lstm.hip, frequency LSTM input DMA (vmcnt 8)",
}
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _tool(name):
    for p in (os.path.join(LLVM, name), shutil.which(name)):
        if p and os.path.exists(p):
            return p
    return None


def _bundles(blob):
    """Every offload bundle in the library (one per HIP source), each cut to its own extent."""
    for m in re.finditer(re.escape(MAGIC), blob):
        s = m.start()
        n, = struct.unpack_from("<Q", blob, s + 24)
        p, end = s + 32, s
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            p += 24 + tl
            end = max(end, s + off + size)
        yield blob[s:end]


def _kernel_metadata():
    """demangled kernel name -> its metadata fields, over every gfx950 code object of the library"""
    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    cxxfilt = _tool("llvm-cxxfilt") or _tool("c++filt")
    if not (bundler and readelf and cxxfilt):
        pytest.skip("needs clang-offload-bundler, llvm-readelf and a demangler (the ROCm LLVM tools)")
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    blob = open(LIB, "rb").read()
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, b in enumerate(_bundles(blob)):
            src, co = os.path.join(tmp, f"b{i}.bundle"), os.path.join(tmp, f"b{i}.co")
            with open(src, "wb") as f:
                f.write(b)
            subprocess.run([bundler, "--unbundle", "--type=o", f"--input={src}", f"--targets={TARGET}", f"--output={co}"], check=True)
            notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
            # one YAML list item per kernel ("  - .agpr_count: ..."), its fields as "    .key: value"
            for item in re.split(r"\n  - ", notes)[1:]:
                fields = dict(re.findall(r"^\s*\.?(\w+):\s+(\S+)$", "  ." + item, re.M))
                if "name" in fields:
                    kernels[fields["name"]] = fields
    names = list(kernels)
    demangled = subprocess.run([cxxfilt], input="\n".join(names), check=True, capture_output=True, text=True).stdout.split("\n")
    # "void (anonymous namespace)::attn_key_score_kernel<1>(AttnKeyArgs)" -> "attn_key_score_kernel<1>"
    plain = lambda d: re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "")).split("(")[0]
    return {plain(d): kernels[n] for n, d in zip(names, demangled)}


def test_counted_wait_kernels_use_no_scratch():
    meta = _kernel_metadata()
    assert len(meta) > 20, sorted(meta)            # the parse found the library's kernels
    bad = {}
    for k, where in COUNTED_WAITS.items():
        found = [name for name in meta if name == k or name.startswith(k + "<")]      # a template name: every instantiation
        assert found, (k, "not in the library", sorted(meta))
        for name in found:
            got = {x: int(meta[name][x]) for x in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
            if any(got.values()):
                bad[name] = (where, got)
    assert not bad, bad
