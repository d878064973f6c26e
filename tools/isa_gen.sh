#!/bin/bash
# tools/isa_gen.sh TREE OUTDIR -- device-only gfx950 assembly of every csrc/*.hip
# of the checkout at TREE, with the Makefile's flags: OUTDIR/prod/ (product
# flags, every file) and OUTDIR/ab/ (-DHPA_AB: the layer, chain, pipe, fused
# and rows files).  Compare two trees with tools/isa_cmp.py.
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
TREE=$1; OUT=$2; mkdir -p "$OUT/prod" "$OUT/ab"
SRC=$TREE/llm.c-paged_amd/csrc
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$TREE/include -I$SRC -Wall -Wno-unused-function -S --offload-device-only"
for f in "$SRC"/*.hip; do
  b=$(basename "$f" .hip); x=""; [ "$b" = hpa_compat ] && x="-ffp-contract=off"
  echo "$HIPCC $FL $x $f -o $OUT/prod/$b.s 2>$OUT/prod/$b.log"
  case $b in hpa_layer*|hpa_chain*|hpa_pipe|hpa_fused|hpa_rows) echo "$HIPCC $FL -DHPA_AB $x $f -o $OUT/ab/$b.s 2>$OUT/ab/$b.log";; esac
done | xargs -P "${JOBS:-8}" -I{} sh -c "{}"
rc=$?  # xargs: 123 if any compile failed
[ $rc -eq 0 ] || { echo "isa_gen.sh: a compile failed; see $OUT/*/*.log" >&2; grep -l "error" "$OUT"/*/*.log >&2; }
exit $rc
