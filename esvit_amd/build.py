"""Build libesvit_hip.so (the C-ABI HIP library) in-tree for gfx950.

    python -m esvit_amd.build [--force]

    python -m esvit_amd.build --variant DIR [--all-hip FLAG ...]     (an A/B build, see build_variant)

hipcc cross-compiles without a GPU, so this runs in the CPU-only container as well as on the
MI355X box.  Objects are cached by mtime and by their compile flags under esvit_amd/csrc/build/;
the shared library is written to esvit_amd/lib/libesvit_hip.so (git-ignored).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJDIR = os.path.join(CSRC, "build")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libesvit_hip.so")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",  # include/esvit_hip.h is the export list
         "-Wno-unused-result", "-I", INCLUDE, "-I", CSRC]
# Extra flags of single sources, appended to FLAGS.  A file is listed here only on a measurement ("build flags"):
# -fno-slp-vectorize keeps adjacent fp32 operations from being packed into v_pk_*_f32, which is slower beside MFMAs and faster away
# from them, so it is decided per file from the kernel times of the training step.
SRC_FLAGS = {
}


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp")))


def _deps_mtime():
    hs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hs.append(os.path.join(INCLUDE, "esvit_hip.h"))
    return max(os.path.getmtime(h) for h in hs)


def _flags(src, src_flags=None):
    """compile flags of one source: the common ones, then the file's own"""
    table = SRC_FLAGS if src_flags is None else src_flags
    return FLAGS + list(table.get(src, []))


def _command(src, obj, src_flags=None):
    return [HIPCC] + _flags(src, src_flags) + ["-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]


def _stamp(obj):
    return obj + ".flags"  # the flags the cached object was compiled with, one per line


def _fresh(src, obj, hdr_mtime, src_flags=None):
    """True if the cached object is newer than the source and the headers AND was compiled with the flags this source has now"""
    path = os.path.join(CSRC, src)
    if not (os.path.exists(obj) and os.path.getmtime(obj) >= os.path.getmtime(path) and os.path.getmtime(obj) >= hdr_mtime):
        return False
    try:
        with open(_stamp(obj)) as f:
            return f.read().split("\n") == _flags(src, src_flags)
    except OSError:
        return False  # (no record of the flags: compile again)


def _compile(src, force, hdr_mtime, objdir=None, src_flags=None):
    obj = os.path.join(objdir or OBJDIR, os.path.splitext(src)[0] + ".o")
    if not force and _fresh(src, obj, hdr_mtime, src_flags):
        return obj, False
    if os.path.exists(_stamp(obj)):
        os.remove(_stamp(obj))
    r = subprocess.run(_command(src, obj, src_flags), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stdout))
    with open(_stamp(obj), "w") as f:
        f.write("\n".join(_flags(src, src_flags)))
    return obj, True


def build(force=False, verbose=True, objdir=None, lib=None, src_flags=None):
    objdir, lib = objdir or OBJDIR, lib or LIB
    os.makedirs(objdir, exist_ok=True)
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    hdr = _deps_mtime()
    srcs = _sources()
    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        results = list(ex.map(lambda s: _compile(s, force, hdr, objdir, src_flags), srcs))
    objs = [o for o, _ in results]
    rebuilt = any(r for _, r in results)
    stale = os.path.exists(lib) and any(os.path.getmtime(o) > os.path.getmtime(lib) for o in objs)  # (an object compiled by hand / by tools/)
    if rebuilt or stale or not os.path.exists(lib) or force:
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s" % r.stdout)
        if verbose:
            print("built", lib)
    elif verbose:
        print("up to date:", lib)
    return lib


def build_variant(outdir, all_hip=(), only=None):
    """An A/B build beside the product: objects and libesvit_hip.so under `outdir`, with the flags `all_hip` appended to every .hip
    file (or to the files named in `only`) on top of SRC_FLAGS.  Load it with ESVIT_HIP_LIB=<outdir>/libesvit_hip.so."""
    table = {s: list(SRC_FLAGS.get(s, [])) for s in _sources()}
    for s in table:
        if s.endswith(".hip") and (only is None or s in only):
            table[s] += [f for f in all_hip if f not in table[s]]
    return build(objdir=os.path.join(outdir, "obj"), lib=os.path.join(outdir, "libesvit_hip.so"), src_flags=table)


if __name__ == "__main__":
    if "--variant" in sys.argv:
        a = sys.argv[1:]
        out = a[a.index("--variant") + 1]
        extra = a[a.index("--all-hip") + 1:] if "--all-hip" in a else []
        build_variant(out, extra)
    else:
        build(force="--force" in sys.argv)
