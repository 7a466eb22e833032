"""csrc/npr_huff.h (the code lengths, their limit, the canonical codes and the length / distance symbols of the device's DEFLATE encoder) on
the host: tests/native/huff_check.cpp, a stand-alone program built with AddressSanitizer and UBSan.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_huffman_parts_of_the_deflate_encoder(tmp_path):
    exe = str(tmp_path / "huff_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nanopore_amd", "csrc"), os.path.join(ROOT, "tests", "native", "huff_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("huff_check ok"), out.stdout + out.stderr
