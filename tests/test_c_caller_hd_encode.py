"""A plain-C caller of the device encoder (tests/c_caller/hd_encode_rig.c): gcc compiles and links it against
include/glc_hd.h and libglc_amd.so; on the GPU it runs the device-only round trip histogram -> table -> encode -> decode."""
import os
import shutil
import subprocess

import pytest

import test_c_caller as TC

RIG = os.path.join(TC.ROOT, "tests", "c_caller", "hd_encode_rig.c")


def test_hd_encode_rig_compiles_with_gcc(glc, tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    glc.lib()
    assert os.path.exists(TC._build(tmp_path, RIG, "hd_encode_rig"))


@pytest.mark.gpu
def test_hd_encode_rig_device_round_trip(glc, tmp_path):
    glc.lib()
    exe = TC._build(tmp_path, RIG, "hd_encode_rig")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "round_trip=1" in r.stdout and "equal_host=1" in r.stdout, r.stdout + r.stderr
