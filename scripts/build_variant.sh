#!/bin/bash
# Build an A/B variant of the library: scripts/build_variant.sh NAME "-DFOO=1 ..." [file.hip ...]
# -> realtimedepthdiffusion_amd/librtdd_NAME.so (the listed .hip files recompiled with the Makefile's flags plus the defines, as
# csrc/<file>.NAME.o; the rest reused); select it at run time with RTDD_LIBRARY=realtimedepthdiffusion_amd/librtdd_NAME.so (a developer
# knob of the Python mirror).
set -e
NAME=$1; DEFS=$2; shift 2
FILES=${@:-sweep_blocked.hip}
cd "$(dirname "$0")/../realtimedepthdiffusion_amd/csrc"
make -j4 >/dev/null
FLAGS=$(make -s --no-print-directory print-cxxflags)
OBJS=""
for f in solver_kernels sweep_blocked rbgs_blocked multigrid image_kernels effect_kernels lens_blur cascade api cascade_api dropin; do
    ext=hip; [ -f $f.cpp ] && ext=cpp
    if echo " $FILES " | grep -q " $f.$ext "; then
        /opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS $DEFS -c $f.$ext -o $f.$NAME.o
        OBJS="$OBJS $f.$NAME.o"
    else
        OBJS="$OBJS $f.o"
    fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../librtdd_$NAME.so $OBJS
echo built librtdd_$NAME.so
