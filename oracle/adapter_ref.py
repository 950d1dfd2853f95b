"""TEST INFRASTRUCTURE ONLY -- adapter/ compiled against the headers of the reference, an Atlas 0.44.1 source checkout, into
oracle/_ref/adapter/ (not committed; tests/test_adapter_source.py inspects it).

For every adapter translation unit, and for tools/adapter_stubs/check_halo_exchange.cc in both halo transports: g++'s front end
(-fsyntax-only) and an object (g++ -c), with tools/adapter_stubs/ supplying only what the checkout lacks (the CMake-generated
headers and declarations of the eckit classes its headers name).  Plus one unit whose override drifts from TransImpl.h (a dropped
const), which the front end must reject.  Return codes and diagnostics go to manifest.json next to the objects, stamped with a
digest of the inputs from this repository.

Run by __graft_entry__.build().  Where the checkout is absent (ATLAS_REFERENCE_SRC, default below) nothing is built and what an
earlier build left stays; the tests skip when there is nothing, and fail when it was built from other sources.

    python oracle/adapter_ref.py"""
import glob
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("ATLAS_REFERENCE_SRC", "/root/reference")
OUT = os.path.join(ROOT, "oracle", "_ref", "adapter")
STUBS = os.path.join(ROOT, "tools", "adapter_stubs")
HALO = os.path.join(STUBS, "check_halo_exchange.cc")
DRIFT = ('#include "TransMI355X.h"\n'
         "struct Drift : atlas::trans::TransMI355X {\n"
         "    using TransMI355X::TransMI355X;\n"
         "    int truncation() override { return 0; }\n"      # TransImpl::truncation() is const
         "};\n")


def units():
    return sorted(glob.glob(os.path.join(ROOT, "adapter", "*.cc")))


def jobs():
    """(object name, source, extra flags)"""
    return [(os.path.basename(u)[:-3], u, []) for u in units()] + \
           [("check_halo_exchange", HALO, []), ("check_halo_exchange_rccl", HALO, ["-DATLAS_AMD_HALO_TRANSPORT_RCCL"])]


def digest():
    """SHA-256 over everything of this repository the compiles read: adapter/, tools/adapter_stubs/, include/, this file"""
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "adapter", "*")) + glob.glob(os.path.join(STUBS, "**", "*"), recursive=True)
                   + glob.glob(os.path.join(ROOT, "include", "*")) + [os.path.abspath(__file__)])
    for f in files:
        if os.path.isfile(f):
            h.update(os.path.relpath(f, ROOT).encode())
            with open(f, "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()


def _gxx(args):
    cmd = ["g++", "-std=c++17", "-Wall", *args, "-I", os.path.join(REFERENCE, "src"), "-I", os.path.join(REFERENCE, "pluto", "src"),
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapter"), "-I", STUBS]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return {"rc": r.returncode, "stderr": r.stderr[-8000:]}


def build():
    if not os.path.isfile(os.path.join(REFERENCE, "src", "atlas", "trans", "detail", "TransImpl.h")):
        print(f"oracle/adapter_ref.py: no Atlas source checkout at {REFERENCE} (ATLAS_REFERENCE_SRC): adapter objects not built")
        return
    manifest = os.path.join(OUT, "manifest.json")
    dg = digest()
    if os.path.exists(manifest):
        with open(manifest) as f:
            if json.load(f).get("digest") == dg:
                return
    os.makedirs(OUT, exist_ok=True)
    out = {"digest": dg, "jobs": {}}
    for name, src, extra in jobs():
        obj = os.path.join(OUT, name + ".o")
        if os.path.exists(obj):
            os.remove(obj)
        out["jobs"][name] = {"extra": extra,
                             "front_end": _gxx(["-fsyntax-only", "-Woverloaded-virtual", *extra, src]),
                             "object": _gxx(["-O0", "-fPIC", "-c", *extra, src, "-o", obj])}
    drift = os.path.join(OUT, "drift.cc")
    with open(drift, "w") as f:
        f.write(DRIFT)
    out["drift"] = _gxx(["-fsyntax-only", "-Woverloaded-virtual", drift])
    with open(manifest, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    sys.exit(build())
