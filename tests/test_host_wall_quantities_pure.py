"""The device-free part of gm_wall_map_quantities (csrc/gm_wall_host.hip: the defaults, the parameter check, one column
restated, the metrics, the runs) on the CPU, under AddressSanitizer and UBSan.

host/gm_wall_quantities_host_test.cpp is a stand-alone program linked with that one source file and nothing else of the
library: it initialises no device and calls no HIP function.  Nothing loaded into Python is sanitised."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_device_free_quantity_calls_run_cleanly_under_sanitizers(tmp_path):
    src = open(os.path.join(ROOT, "geometric_mapping_amd", "csrc", "gm_wall_host.hip")).read()
    assert re.search(r"\bhip[A-Z]\w*\s*\(", src) is None   # the file calls no HIP function
    for name in ("gm_wall_quantity_default_params", "gm_wall_quantity_check_params", "gm_wall_quantity_column",
                 "gm_wall_quantity_metrics", "gm_wall_quantity_runs"):
        assert re.search(r"\b%s\s*\(" % name, src), name
    exe = str(tmp_path / "gm_wall_quantities_host_test")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    subprocess.run([os.path.join(ROCM, "bin", "hipcc"), "--offload-host-only", "-std=c++17", "-O1", "-g"] + san +
                   [os.path.join(ROOT, "geometric_mapping_amd", "csrc", "gm_wall_host.hip"),
                    os.path.join(ROOT, "host", "gm_wall_quantities_host_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("gm_wall_quantities_host_test ok"), r.stdout + r.stderr
