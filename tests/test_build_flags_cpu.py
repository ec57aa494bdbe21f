"""The per-source compile flags of esvit_amd/build.py (no GPU, no compiler run): every key of SRC_FLAGS names a source of csrc/, the
command of such a file carries its own flags after every common flag, and a cached object goes stale when its file's entry changes."""
import os
import time

from esvit_amd import build as B


def test_every_key_names_a_source():
    srcs = set(B._sources())
    for key, flags in B.SRC_FLAGS.items():
        assert key in srcs, "SRC_FLAGS names %r, which is no source file of esvit_amd/csrc" % key
        assert isinstance(flags, (list, tuple)) and all(isinstance(f, str) and f.startswith("-") for f in flags), (key, flags)


def _check_command(src, table, extra):
    obj = os.path.join(B.OBJDIR, os.path.splitext(src)[0] + ".o")
    cmd = B._command(src, obj, table)
    assert cmd[0] == B.HIPCC and cmd[-6:] == ["-x", "hip", "-c", os.path.join(B.CSRC, src), "-o", obj]
    flags = cmd[1:-6]
    assert flags[:len(B.FLAGS)] == B.FLAGS, "a common flag is missing from the command of %s" % src
    assert flags[len(B.FLAGS):] == list(extra), "the flags of %s: %r, expected %r" % (src, flags[len(B.FLAGS):], extra)


def test_commands_carry_the_common_flags_and_their_own():
    for src in B._sources():  # the committed table, file by file
        _check_command(src, None, B.SRC_FLAGS.get(src, []))
    src = "mlp_fused16.hip"  # and a table of the test's own
    assert src in B._sources()
    _check_command(src, {src: ["-fno-slp-vectorize", "-DX=1"]}, ["-fno-slp-vectorize", "-DX=1"])
    _check_command("gemm.hip", {src: ["-fno-slp-vectorize"]}, [])


def test_a_changed_entry_invalidates_the_cached_object(tmp_path):
    src = "mlp_fused16.hip"
    obj = str(tmp_path / "mlp_fused16.o")
    with open(obj, "w") as f:
        f.write("object")
    newer = max(os.path.getmtime(os.path.join(B.CSRC, src)), B._deps_mtime(), time.time()) + 10
    os.utime(obj, (newer, newer))
    assert not B._fresh(src, obj, B._deps_mtime(), {}), "an object with no record of its flags counts as fresh"
    with open(B._stamp(obj), "w") as f:
        f.write("\n".join(B._flags(src, {})))
    assert B._fresh(src, obj, B._deps_mtime(), {})
    assert B._fresh(src, obj, B._deps_mtime(), {"gemm.hip": ["-fno-slp-vectorize"]}), "another file's entry invalidated this one"
    assert not B._fresh(src, obj, B._deps_mtime(), {src: ["-fno-slp-vectorize"]}), "a new entry did not invalidate the object"
    with open(B._stamp(obj), "w") as f:
        f.write("\n".join(B._flags(src, {src: ["-fno-slp-vectorize"]})))
    assert B._fresh(src, obj, B._deps_mtime(), {src: ["-fno-slp-vectorize"]})
    assert not B._fresh(src, obj, B._deps_mtime(), {src: ["-fno-slp-vectorize", "-O2"]}), "a changed entry did not invalidate the object"
    assert not B._fresh(src, obj, B._deps_mtime(), {}), "a removed entry did not invalidate the object"
    old = os.path.getmtime(os.path.join(B.CSRC, src)) - 10  # (the mtime rule still holds beside the flags)
    os.utime(obj, (old, old))
    assert not B._fresh(src, obj, B._deps_mtime(), {src: ["-fno-slp-vectorize"]})
