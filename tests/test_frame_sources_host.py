"""CPU: which files the frame kernels' source hash covers (``ops.FRAME_KERNEL_SOURCES``: a PMC traffic record of bench.py stays
paired with the code it measured, and only with that). Reads source text only."""
import os
import re
import shutil

from conftest import ROOT
from tarl_hip import ops

CSRC = os.path.join(ROOT, "tarl-simulator_amd", "csrc")
FRAME_FILES = ("fused_direction.hip", "fused_rows.hip", "fused_insert.hip")
FRAME_KERNELS = ("k_fused_direction", "k_fused_rows", "k_fused_insert", "k_fused_insert2", "k_fused_insert_choice")


def quoted_includes(name):
    """The csrc files a csrc file includes with quotes (an include that leaves the directory, the public header, is not one)."""
    text = open(os.path.join(CSRC, name)).read()
    return [inc for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M) if "/" not in inc]


def test_every_included_header_is_hashed():
    assert ops.FRAME_KERNEL_SOURCES[:3] == FRAME_FILES
    todo, seen = list(FRAME_FILES), set()
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        assert name in ops.FRAME_KERNEL_SOURCES, f"{name} is compiled into a frame kernel but not hashed"
        todo += quoted_includes(name)
    assert seen == set(ops.FRAME_KERNEL_SOURCES), f"hashed but not included: {set(ops.FRAME_KERNEL_SOURCES) - seen}"
    for name in ops.FRAME_KERNEL_SOURCES:
        assert os.path.isfile(os.path.join(CSRC, name)), name


def test_each_frame_kernel_is_defined_once_in_a_hashed_file():
    sources = {n: open(os.path.join(CSRC, n)).read() for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".h"))}
    for kernel in FRAME_KERNELS:
        where = [n for n, text in sources.items()
                 if re.search(r"__global__[^;{]*?\bvoid\s+" + kernel + r"\s*\(", text, flags=re.S)]
        assert len(where) == 1, f"{kernel} defined in {where}"
        assert where[0] in ops.FRAME_KERNEL_SOURCES, f"{kernel} lives in {where[0]}, which the hash does not cover"
    assert not os.path.exists(os.path.join(CSRC, "fused.hip"))


def test_hash_follows_its_members_only(tmp_path):
    d = str(tmp_path)
    for name in ops.FRAME_KERNEL_SOURCES + ("fused_pack.hip",):
        shutil.copy(os.path.join(CSRC, name), d)
    h0 = ops.frame_kernel_source_hash(d)
    assert h0 == ops.frame_kernel_source_hash() and re.fullmatch(r"[0-9a-f]{16}", h0)
    with open(os.path.join(d, "fused_pack.hip"), "ab") as fh:
        fh.write(b"// a comment\n")
    assert ops.frame_kernel_source_hash(d) == h0, "pack is not part of what a traffic record measured"
    for name in ops.FRAME_KERNEL_SOURCES:
        path = os.path.join(d, name)
        data = open(path, "rb").read()
        open(path, "wb").write(data[:-1] + bytes([data[-1] ^ 1]))
        assert ops.frame_kernel_source_hash(d) != h0, f"one byte of {name} changed and the hash did not"
        open(path, "wb").write(data)
    assert ops.frame_kernel_source_hash(d) == h0
