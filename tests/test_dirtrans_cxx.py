"""tests/cpp/test_dirtrans_cxx.cc: the direct transform through include/atlas_amd.hpp, compiled with g++ against the shared
library (as tests/test_cxx_api.py builds its callers) and run on the GPU: an F32 round trip."""
import os
import subprocess

import pytest

from atlas_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cxx_binary(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cxx_dirtrans") / "test_dirtrans_cxx")
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_dirtrans_cxx.cc"), "-o", out,
           "-L", libdir, "-latlas_amd", f"-Wl,-rpath,{libdir}", "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cxx_dirtrans_caller_compiles(cxx_binary):
    assert os.access(cxx_binary, os.X_OK)


@pytest.mark.gpu
def test_cxx_dirtrans_round_trip_f32(cxx_binary):
    r = subprocess.run([cxx_binary], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failure(s)" in r.stdout
