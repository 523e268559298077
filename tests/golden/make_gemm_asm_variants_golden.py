"""Writes gemm_asm_variants_v1.json: sha256 of what the assembly GEMM generator of commit a8e35a8 (the last one before
tools/gen_gemm_asm.py became an importable module) writes under every schedule option that was kept.  The hashes pin the
refactored generator to its predecessor, so they come from that commit's script, never from the current one:

    python tests/golden/make_gemm_asm_variants_golden.py
"""
import hashlib
import json
import os
import pathlib
import subprocess
import sys
import tempfile

PARENT = "a8e35a8"
VARIANTS = ["default", "ASM_RING=0", "ASM_STORE_NT=0", "ASM_RD_STRIDE=3", "ASM_DMA_STRIDE=2"] + \
    [f"ASM_ABL={t}" for t in ("m32", "nodma", "noread", "gll", "spread", "nowait", "nobar", "nomath", "nostore", "nodma+nowait+nobar")]

if __name__ == "__main__":
    here = pathlib.Path(__file__).resolve().parent
    src = subprocess.run(["git", "show", f"{PARENT}:tools/gen_gemm_asm.py"], cwd=here, capture_output=True, check=True).stdout
    base = {k: v for k, v in os.environ.items() if not k.startswith("ASM_")}
    out = {}
    with tempfile.TemporaryDirectory() as td:
        script = pathlib.Path(td) / "gen_gemm_asm.py"
        script.write_bytes(src)
        for v in VARIANTS:
            env = dict(base, **dict([v.split("=", 1)])) if v != "default" else base
            out[v] = hashlib.sha256(subprocess.run([sys.executable, str(script)], capture_output=True, check=True, env=env).stdout).hexdigest()
    (here / "gemm_asm_variants_v1.json").write_text(json.dumps(out, indent=1) + "\n")
