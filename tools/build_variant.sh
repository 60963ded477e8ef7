#!/bin/bash
# Build an experimental variant of libaurora_hip.so:  tools/build_variant.sh <name> [extra hipcc flags for the gemm*.hip files ...]
# -> aurora_amd/_lib/libaurora_hip_<name>.so   (select with AURORA_HIP_LIB=<path>)
set -e
NAME=$1; shift
D=aurora_amd/_lib/var_$NAME; mkdir -p $D aurora_amd/_lib/var_cache
CC="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -amdgpu-mfma-vgpr-form=1"
for src in aurora_amd/csrc/*.hip; do
  f=$(basename $src .hip)
  case $f in
    gemm*) $CC "$@" -c $src -o $D/$f.o & ;;
    *) if [ ! -f aurora_amd/_lib/var_cache/$f.o ] || [ $src -nt aurora_amd/_lib/var_cache/$f.o ]; then
         $CC -c $src -o aurora_amd/_lib/var_cache/$f.o &
       fi ;;
  esac
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC aurora_amd/_lib/var_cache/*.o $D/*.o -o aurora_amd/_lib/libaurora_hip_$NAME.so
rm -rf $D
echo built aurora_amd/_lib/libaurora_hip_$NAME.so
