#!/bin/bash
# device_asm.sh -- the device assembly of every csrc/*.hip of a checkout, with the library's flags (lidar_transfer_amd/build.py:
# FLAGS without -shared, the two -I) plus --cuda-device-only -S, and its SHA-256 per file.  No GPU needed.  For a change that
# must not touch a kernel: run it on a checkout of the parent commit and on the tree, the two listings must be equal.
#   tools/device_asm.sh <checkout> <outdir>
# hipcc names one symbol per file (__hip_cuid_*) after a hash of its command line, so every checkout is compiled at the SAME
# place into the SAME place: copied to $TMPDIR/lidarhip_devasm, assembled into asm/ there, moved to <outdir> afterwards.
set -o pipefail
tree=$(cd "$1" && pwd) || exit 2
mkdir -p "$2" && out=$(cd "$2" && pwd) || exit 2
w=${TMPDIR:-/tmp}/lidarhip_devasm
rm -rf "$w" && mkdir -p "$w/asm" "$w/lidar_transfer_amd" || exit 2
cp -r "$tree/include" "$w/" && cp -r "$tree/lidar_transfer_amd/csrc" "$w/lidar_transfer_amd/" && cd "$w" || exit 2
hipcc=$(command -v hipcc || echo /opt/rocm/bin/hipcc)
fail=0
for f in lidar_transfer_amd/csrc/*.hip; do
  b=$(basename "$f" .hip)
  "$hipcc" --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-result -fno-slp-vectorize \
    -I include -I lidar_transfer_amd/csrc --cuda-device-only -S -o "asm/$b.s" "$f" 2> "asm/$b.err" || { echo "FAILED $b" >&2; fail=1; }
done
mv asm/* "$out"/ && cd "$out" && sha256sum *.s
exit $fail
