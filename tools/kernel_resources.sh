#!/bin/bash
# Build container (no GPU): registers, occupancy and SPILLS of every kernel of libl2i_hip.so from the compiler's resource report
# (hipcc -Rpass-analysis=kernel-resource-usage), one line per kernel; kernels with spilled registers are marked.  Run before collecting profiles:
# a spilled register is scratch traffic that the PMC passes count as HBM bytes of the launch ("A correction ...").
# Compiler, flags and the list of objects (the _f16 twins included) are the Makefile's own (`make flags`).
#   bash tools/kernel_resources.sh [--spills]      (--spills: only the kernels that spill)
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R/latent2im_amd/csrc
ONLY=${1:-}
HIPCC=$(make -s flags | sed -n 's/^HIPCC=//p'); CXXFLAGS=$(make -s flags | sed -n 's/^CXXFLAGS=//p')
for o in $(make -s flags | sed -n 's/^OBJS=//p'); do
  stem=${o%.o}; def=""
  case "$stem" in *_f16) def="-DL2I_H8_F16" ;; esac
  f=${stem%_f16}.hip
  $HIPCC $CXXFLAGS $def -cuid=$stem -Rpass-analysis=kernel-resource-usage -c $f -o /dev/null 2>&1 |
    grep -E "Function Name|VGPRs:|AGPRs:|VGPRs Spill|Occupancy|LDS Size" | paste - - - - - - |
    sed "s/$f:[0-9:]* remark: *//g; s/\[-Rpass-analysis=kernel-resource-usage\]//g; s/Function Name: //; s/  */ /g" |
    awk -v only="$ONLY" -v file="$f$def" '{ spill = ($0 !~ /VGPRs Spill: 0 /); if (only != "--spills" || spill) print (spill ? "SPILL " : "      ") file " " $0 }'
done
