"""Static instruction counts of the persistent GEMM's epilogue region (csrc/include/gemm_pk.h).

Usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=fast -munsafe-fp-atomics -Icsrc/include \
           -S --offload-device-only csrc/kernels/gemm_pk_tt.hip -o tt.s
       python scripts/gemm_epilogue_count.py tt.s [more .s files]

For every gemm_pk instance: the instructions in program order between the last MFMA of the tile loop
and the last buffer store of the kernel (the epilogue of one tile, per wave), by class.  The counts are
of the emitted code; a launch executes fewer where the region still branches on its arguments (the
PK_EPI_ANY instances), so the table also gives the conditional branches.
"""
import re
import sys

NAME = re.compile(r"gemm_pkILb(\d)ELb(\d)ELi(\d+)ELb(\d)ELb(\d)ELi(\d+)ELi(\d+)ELb(\d)(?:ELi(n?\d+))?E")


def kernels(path):
    body, name = None, None
    for line in open(path):
        m = re.match(r"^(_ZN14rn_gemm_detail7gemm_pk\S+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if body is not None:
            if line.startswith("\t.section") or line.lstrip().startswith(".amdhsa_kernel") or line.startswith(".Lfunc_end"):
                yield name, body
                body = None
                continue
            body.append(line.split(";")[0].strip())


def count(body):
    ins = [l for l in body if l]
    last_mfma = max(i for i, l in enumerate(ins) if l.startswith("v_mfma"))
    last_store = max(i for i, l in enumerate(ins) if l.startswith("buffer_store"))
    reg = ins[last_mfma + 1:last_store + 1]
    c = dict(blocks=0, valu=0, salu=0, stores=0, loads=0, cbranch=0, v_mov=0, s_nop=0)
    for l in reg:
        op = l.split()[0]
        if op.endswith(":"):
            c["blocks"] += 1
        elif op.startswith("buffer_store"):
            c["stores"] += 1
        elif op.startswith(("buffer_load", "global_load", "s_load", "s_buffer_load")):
            c["loads"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            c["v_mov"] += op == "v_mov_b32_e32" or op == "v_mov_b32"
        elif op.startswith("s_"):
            c["salu"] += 1
            c["cbranch"] += op.startswith("s_cbranch")
            c["s_nop"] += op == "s_nop"
    return c


def main():
    print(f"{'file':<22}{'AK BK ACT SPL F32 DBG FP8 DYN EPI':<36}" + "".join(f"{k:>8}" for k in
          ("blocks", "valu", "salu", "stores", "loads", "cbranch", "v_mov", "s_nop")))
    for path in sys.argv[1:]:
        for name, body in kernels(path):
            g = NAME.search(name).groups()
            tag = " ".join(f"{(x or 'any').replace('n1', 'any'):>3}" for x in g)
            c = count(body)
            print(f"{path.split('/')[-1]:<22}{tag:<36}" + "".join(f"{v:>8}" for v in c.values()))


if __name__ == "__main__":
    main()
