#!/bin/bash
# A variant of the library for A/B runs, fast: only the units that hold the tabulation and rescale kernels (mdx_kernels.hip,
# mdx_rescale.hip: every MDX_* / RS_* knob is theirs) are compiled afresh, with the flags given; the other objects are the
# in-tree build's (mapdamage_amd/build/obj), the list mapdamage_amd.build.SOURCES.
# usage: tools/mkv.sh <tag> [-DMDX_...=...]  -> tools/bin/libmdx_<tag>.so
set -e
cd "$(dirname "$0")/.."
tag=$1; shift
mkdir -p tools/bin
S=mapdamage_amd/csrc; O=mapdamage_amd/build/obj
objs=
for src in $(python -c "from mapdamage_amd.build import SOURCES; print(' '.join(SOURCES))"); do
  case $src in
    mdx_kernels.hip|mdx_rescale.hip)
      hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -x hip -Wall -Wno-unused-function "$@" -c $S/$src -o tools/bin/${src}_$tag.o
      objs="$objs tools/bin/${src}_$tag.o";;
    *) objs="$objs $O/$src.o";;
  esac
done
hipcc --offload-arch=gfx950 -fPIC -shared $objs -lz -lpthread -ldl -o tools/bin/libmdx_$tag.so
rm -f tools/bin/mdx_kernels.hip_$tag.o tools/bin/mdx_rescale.hip_$tag.o
echo "built tools/bin/libmdx_$tag.so ($*)"
