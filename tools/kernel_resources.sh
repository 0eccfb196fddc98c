#!/bin/bash
# usage: tools/kernel_resources.sh prnn   -> compact VGPR/AGPR/scratch/occupancy table for one TU, compiled with the flags build.py
# gives that file (build.compile_flags: no second copy of them here)
# targets: any translation unit of build.SOURCES without its suffix - prnn, lstm, lstm_grad, lstm_pauli (the LSTM's Pauli pass: its
# table is profiles/lstm_pauli_kernel_resources.txt, zero scratch at every NFULL is a condition of that pass), lstm_renyi (the LSTM's
# region-Renyi pass: the PAIRED tails, profiles/lstm_renyi_kernel_resources.txt puts them beside lstm_pauli's !PAIRED rows; zero
# scratch at every NFULL is a condition of that pass too), ...
f=${1:-prnn}
cd "$(dirname "$0")/.." || exit 1
flags=$(python3 -c 'import sys; from rnnwavefunctions_amd import build; print(" ".join(build.compile_flags(sys.argv[1] + ".hip")))' "$f") || exit 1
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
${HIPCC:-/opt/rocm/bin/hipcc} $flags --cuda-device-only -Rpass-analysis=kernel-resource-usage -c rnnwavefunctions_amd/csrc/$f.hip -o $out/$f.o 2>&1 |
python3 -c '
import sys,re,subprocess
cur=None; rows=[]
for line in sys.stdin:
    m=re.search(r"remark: [^:]*:\d+:\d+: +(.*?) \[-Rpass", line) or re.search(r"remark: +(.*?) \[-Rpass", line)
    if not m:
        m2=re.search(r": +(Function Name|Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|SGPRs|VGPR Spill|SGPR Spill): (.*?) \[", line)
        if not m2: continue
        k,v=m2.group(1),m2.group(2)
    else:
        kv=m.group(1).split(": ")
        if len(kv)<2: continue
        k,v=kv[0].strip(),kv[1].strip()
    if k in ("Function Name","Name"):
        cur={"name":v}; rows.append(cur)
    elif cur is not None: cur[k]=v
for r in rows:
    n=subprocess.run(["c++filt",r["name"]],capture_output=True,text=True).stdout.strip().split("(")[0]
    print("%-62s V=%-4s A=%-4s S=%-4s scratch=%-4s occ=%s" % (n[-62:], r.get("VGPRs"), r.get("AGPRs"), r.get("SGPRs", r.get("TotalSGPRs")), r.get("ScratchSize [bytes/lane]"), r.get("Occupancy [waves/SIMD]")))
'
