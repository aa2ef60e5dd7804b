"""Gene::merge_targets() through the C++ facade: the constructor's save_umi_merge_targets reaches the container
(tests/cpp/umi_merge_targets.cpp)."""
import subprocess

import pytest

from dropest_amd.build import UMI_TARGETS_TOOL, build_facade

pytestmark = pytest.mark.gpu


def test_the_facade_keeps_umi_merge_targets_when_asked():
    build_facade()
    res = subprocess.run([UMI_TARGETS_TOOL], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "umi merge targets ok" in res.stdout
