#!/bin/bash
# usage: tools/ab_build.sh <tag> [extra hipcc flags, e.g. -DSDM_X=1]  ->  build/ab/libsdm_<tag>.so
# A/B variants of the library for one and the same GPU run (box-to-box spread is a few percent: variants are only
# comparable inside one gpurun call); load one with SDM_LIB_PATH=build/ab/libsdm_<tag>.so.
# Sources and flags are csrc/Makefile's; the variant's objects are built out of tree, the default build is not touched.
set -e
tag=$1; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
make -s -j8 -C "$root/semantic_dsp_map_amd/csrc" LIB="$root/build/ab/libsdm_$tag.so" OBJDIR="$root/build/ab/obj_$tag" EXTRA="$*"
rm -rf "$root/build/ab/obj_$tag"
echo built build/ab/libsdm_$tag.so
