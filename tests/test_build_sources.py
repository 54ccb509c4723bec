"""The build recipe's file lists against the files of csrc/ (no GPU, no compiler)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcquic_amd", "csrc")


def _included(path):
    """Quoted includes of `path` (resolved against its directory), transitively."""
    out, todo = set(), [path]
    while todo:
        f = todo.pop()
        for inc in re.findall(r'#\s*include\s+"([^"]+)"', open(f).read()):
            g = os.path.normpath(os.path.join(os.path.dirname(f), inc))
            if g not in out:
                out.add(g)
                todo.append(g)
    return out


def test_every_source_of_the_build_exists():
    from mcquic_amd import build as B
    assert len(set(B.SOURCES)) == len(B.SOURCES)
    missing = [s for s in B.SOURCES if not os.path.isfile(os.path.join(B.CSRC, s))]
    assert not missing, f"build.SOURCES names files that are not in csrc/: {missing}"
    unbuilt = [f for f in os.listdir(B.CSRC) if f.endswith((".hip", ".cpp")) and f not in B.SOURCES]
    assert not unbuilt, f"sources in csrc/ that build.SOURCES does not compile: {unbuilt}"


def test_conv_stamp_covers_every_file_of_the_conv_kernel():
    """csrc_sha() is what the counter passes under profiles/ are stamped with (bench.py: traffic_stale).  Every file of csrc/ that
    names conv_mfma_kernel, and every file such a file includes, must be part of it -- wherever the next file move puts them."""
    from mcquic_amd import build as B
    assert os.path.samefile(B.CSRC, CSRC)
    needed = set()
    for name in os.listdir(CSRC):
        path = os.path.join(CSRC, name)
        if os.path.isfile(path) and "conv_mfma_kernel" in open(path, errors="replace").read():
            needed |= {path} | _included(path)
    assert len(needed) >= 8, "the kernel header, its instance units, the launcher and the pack file at least"
    covered = {os.path.normpath(f) for f in B.conv_files()}
    assert all(os.path.isfile(f) for f in covered)
    left_out = sorted(os.path.relpath(f, ROOT) for f in needed - covered)
    assert not left_out, f"hold or feed conv_mfma_kernel but are outside csrc_sha(): {left_out}"
    assert re.fullmatch(r"[0-9a-f]{64}", B.csrc_sha())
