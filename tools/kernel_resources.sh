#!/bin/bash
# Developer tool: register / spill / scratch figures of the frame kernels' bench instantiations, from the compiler's own
# resource remarks (-Rpass-analysis=kernel-resource-usage) and the static instruction mix of the device ISA (--save-temps).
# usage: tools/kernel_resources.sh [extra hipcc flags]   (run from anywhere; writes nothing into the tree)
#        default SRC: the three frame-kernel files, fused_direction.hip fused_rows.hip fused_insert.hip
#        SRC=occupancy.hip tools/kernel_resources.sh    every kernel of another file of csrc/, under its mangled name
#        SRC=trips.hip tools/kernel_resources.sh        (the per-trip reductions: the figures of DESIGN 4.16)
cd "$(dirname "$0")/../tarl-simulator_amd/csrc"
T=$(mktemp -d)
FRAME="fused_direction.hip fused_rows.hip fused_insert.hip"
for f in ${SRC:=$FRAME}; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Rpass-analysis=kernel-resource-usage \
    --save-temps=obj "$@" -c $f -o $T/${f%.hip}.o 2>> $T/remarks.txt
done
python3 - $T "$SRC" "$FRAME" <<'PY'
import re, sys, glob
T = sys.argv[1]
want = {"_Z12k_fused_rowsILi4ELb1ELb0ELb1EE": "k_fused_rows<4,SIB,rollout,O32>", "_Z17k_fused_directionILi4ELb1ELb1ELb1EE": "k_fused_direction<4,SIB,CNT,O32>",
        "_Z15k_fused_insert2ILi8ELb0EE": "k_fused_insert2<8,noLP>", "_Z15k_fused_insert2ILi8ELb1EE": "k_fused_insert2<8,LP>",
        "_Z15k_fused_insert2ILi2ELb0EE": "k_fused_insert2<2,noLP>",
        "_Z15k_fused_insert2ILi2ELb1EE": "k_fused_insert2<2,LP>", "_Z15k_fused_insert2ILi4ELb0EE": "k_fused_insert2<4,noLP>",
        "_Z15k_fused_insert2ILi4ELb1EE": "k_fused_insert2<4,LP>", "_Z14k_fused_insertILb0EE": "k_fused_insert<noLP>",
        "_Z14k_fused_insertILb1EE": "k_fused_insert<LP>", "_Z21k_fused_insert_choiceILb0EE": "k_fused_insert_choice<noLP>",
        "_Z21k_fused_insert_choiceILb1EE": "k_fused_insert_choice<LP>"}
txt = open(T + "/remarks.txt").read()
blocks = re.split(r"Function Name: ", txt)[1:]
if sys.argv[2] != sys.argv[3]:
    want = {b.split()[0]: b.split()[0][:36] for b in blocks}
res = {}
for b in blocks:
    name = b.split()[0]
    for k, nice in want.items():
        if name.startswith(k):
            g = lambda pat, b=b: (re.search(pat + r": (\d+)", b) or [None, "?"])[1]
            res[nice] = dict(sgpr=g("TotalSGPRs"), vgpr=g("VGPRs"), sspill=g("SGPRs Spill"), vspill=g("VGPRs Spill"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                             occ=g(r"Occupancy \[waves/SIMD\]"), lds=g(r"LDS Size \[bytes/block\]"))
mix = {}
for asm in glob.glob(T + "/*gfx950*.s"):
    cur = None
    for line in open(asm):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = next((nice for k, nice in want.items() if m.group(1).startswith(k)), None)
            if cur:
                mix[cur] = dict(valu=0, salu=0, vmem=0, smem=0, lds=0, lanespill=0, flat=0)
            continue
        if cur is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
            continue
        op = line.strip().split(" ")[0].split("\t")[0]
        if op.startswith("v_readlane") or op.startswith("v_writelane"):
            mix[cur]["lanespill"] += 1
        if op.startswith("v_"):
            mix[cur]["valu"] += 1
        elif op.startswith("s_load") or op.startswith("s_buffer_load"):
            mix[cur]["smem"] += 1
        elif op.startswith("s_"):
            mix[cur]["salu"] += 1
        elif op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_") or op.startswith("scratch_"):
            mix[cur]["vmem"] += 1
            if op.startswith("flat_"):      # an access without an address space (a pointer that was loaded from memory)
                mix[cur]["flat"] += 1
        elif op.startswith("ds_"):
            mix[cur]["lds"] += 1
print(f"{'kernel':36s} {'SGPR':>4s} {'VGPR':>4s} {'sSpill':>6s} {'vSpill':>6s} {'scratch':>7s} {'occ':>3s} {'LDS':>6s} | static: {'VALU':>5s} {'SALU':>5s} {'SMEM':>4s} {'VMEM':>4s} {'FLAT':>4s} {'DS':>3s} {'v_read/writelane':>16s}")
for nice in want.values():
    if nice in res:
        r, m = res[nice], mix.get(nice, {})
        print(f"{nice:36s} {r['sgpr']:>4s} {r['vgpr']:>4s} {r['sspill']:>6s} {r['vspill']:>6s} {r['scratch']:>7s} {r['occ']:>3s} {r['lds']:>6s} | "
              f"        {m.get('valu', 0):5d} {m.get('salu', 0):5d} {m.get('smem', 0):4d} {m.get('vmem', 0):4d} {m.get('flat', 0):4d} {m.get('lds', 0):3d} {m.get('lanespill', 0):16d}")
PY
rm -rf $T
