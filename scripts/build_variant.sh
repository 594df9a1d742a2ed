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
# the library's sources are the Makefile's own list: a new translation unit is linked into every variant too
for src in $(make -s --no-print-directory print-srcs); do
    f=${src%.*}; ext=${src##*.}
    if echo " $FILES " | grep -q " $f.$ext "; then
        /opt/rocm/bin/hipcc --offload-arch=gfx950 $FLAGS $DEFS -c $f.$ext -o $f.$NAME.o
        OBJS="$OBJS $f.$NAME.o"
    else
        OBJS="$OBJS $f.o"
    fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,-z,defs -o ../librtdd_$NAME.so $OBJS
echo built librtdd_$NAME.so
