"""host/gm_cloud_output_test: the page-locked /choppedCloud rows of Processor::enableCloudOutput when a larger frame is
submitted while an earlier one is in flight.  A Processor with two slots and 1 000 rows takes an 800-point frame A and a
6 000-point frame B with no wait in between; both clouds must equal, row for row, what processFrame returns for A and
for B alone -- on one context with two slots and on two ranks that share a device.  Before the rows a frame wrote into
were kept with the frame, the first comparison failed: growing the buffers for B freed A's rows, and choppedCloud() copied
A's n_valid rows out of the new, never-written buffer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "host", "gm_cloud_output_test")


def test_cloud_output_test_builds_with_plain_gxx():
    subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_cloud_output_test"], check=True, capture_output=True)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_clouds_of_frames_in_flight_survive_growth_on_gpu():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "gm_cloud_output_test"], check=True, capture_output=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gm_cloud_output_test ok" in r.stdout
