"""Records tests/golden/gemm_bits_v1.json: what the HIP GEMM kernels write, bit for bit, on the cases of tests/test_gemm_bits_gpu.py
(sha256 per output buffer) with the sha256 of every seeded input block.  Needs the GPU.

The committed fixture was taken at the commit it names, the last one whose gemm.hip stated the epilogue arithmetic four times, the
256 x 256 launcher five times and the operand staging once per kernel; two recordings there were byte-equal.  It is not meant to be
regenerated from the current tree: only a change that MEANS to move the bits (another summation order, another rounding point)
records it again, from the tree it leaves, and says so.

  python tests/golden/make_gemm_bits_golden.py <commit> [<output file>]
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import torch

from lap_amd import hip
from tests import test_gemm_bits_gpu as T


def main():
    scratch = T.make_scratch()
    results = {}
    for group in T.GROUPS:
        results.update(T.group_results(hip, group, scratch))
    torch.cuda.synchronize()
    fixture = {"commit": sys.argv[1], "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "inputs": T.input_hashes(),
               "results": results}
    out = pathlib.Path(sys.argv[2]) if len(sys.argv) > 2 else T.FIXTURE
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(fixture, indent=1) + "\n")
    print(len(results), "cases ->", out)


if __name__ == "__main__":
    main()
