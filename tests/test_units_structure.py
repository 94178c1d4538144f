"""The API unit holds host code only: every kernel is defined and launched in the unit of its family, behind a launch_* of
h2r_internal.hpp.  Read from the sources; nothing is compiled."""
import glob
import os
import re

from halo2_rsa_amd import _build


def _read(path):
    with open(path) as f:
        return f.read()


def test_the_api_unit_defines_and_launches_no_kernel():
    api = _read(os.path.join(_build.CSRC, "h2r_api.hip"))
    for word in ("__global__", "LaunchKernelGGL", "H2R_TU_API"):
        assert api.count(word) == 0, word


def test_no_source_knows_an_api_unit_guard():
    for path in glob.glob(os.path.join(_build.CSRC, "*")):
        assert "H2R_TU_API" not in _read(path), path


def test_every_unit_is_in_the_list_of_the_internal_header():
    head = _read(os.path.join(_build.CSRC, "h2r_internal.hpp")).split("#pragma once")[0]
    listed = set(re.findall(r"h2r_\w+\.hip", head))
    assert len(set(_build.UNITS)) == len(_build.UNITS)
    for unit in _build.UNITS:
        assert unit in listed, unit
