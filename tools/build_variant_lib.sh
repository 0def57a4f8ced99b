#!/bin/bash
# Build a variant libpt2q.so (build container) from a scratch copy of the package sources with extra
# compiler flags -- a probe mask of csrc/probe.hpp, e.g. -DPT2Q_EF2_KPROBE=4 or -DPT2Q_ATQ_KPROBE=8 --
# into tools/_gx/lib_NAME.so, where tools/inv_lib_ab.sh looks for variants and tools/lib_ab.sh can
# take it as OLD_SO.  The in-tree build is left alone.
#   bash tools/build_variant_lib.sh NAME [FLAGS...]
set -e
NAME=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
P=$R/snlp---tenary-post-train-quantization_amd
T=$(mktemp -d /tmp/pt2q_var.XXXX)
mkdir -p $T/pkg $R/tools/_gx
cp -r $P/csrc $P/Makefile $T/pkg/
ln -s $R/include $T/include
make -s -C $T/pkg -j16 EXTRA_HIPFLAGS="$*"
cp $T/pkg/libpt2q.so $R/tools/_gx/lib_$NAME.so
rm -rf $T
