"""Builds libpredictor_emu.so: csrc/predictor_rows.hip (the thin projection and the thin embedding of a temporal predictor with
their gradients and sums; wave sums by __shfl_xor, no MFMA) compiled FOR THE HOST against the stand-in HIP header of this directory
(test infrastructure only; see hip/hip_runtime.h and build_emu.py)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SOURCES = [os.path.join(ROOT, "tacotron2_amd", "csrc", "predictor_rows.hip"), os.path.join(HERE, "emu_runtime.cpp")]


def build(out_dir, verbose=False):
    out = os.path.join(out_dir, "libpredictor_emu.so")
    cmd = ["g++", "-std=c++17", "-O1", "-g0", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
           "-I", HERE, "-x", "c++"] + SOURCES + ["-o", out]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    import tempfile
    print(build(tempfile.mkdtemp(), verbose=True))
