#!/bin/bash
# A/B of library builds on one box: tools/ab.sh "<kbench args>" name1 name2 ...   ("-" = the shipping library);
# two interleaved rounds.  `name` is the VARIANT of `make -C acfm_video_3d_reconstruction_amd/csrc VARIANT=name [EXTRA="-D..."]`
# (-> libacfm_hip_name.so beside the shipping library: build one before an edit and one after it).  The named -D switches
# of the earlier rounds were removed with the code they selected (verdicts: DESIGN.md section 5, code: tools/variants/).
# tools/isa_diff.py shows which kernels two builds actually differ in.
args="$1"; shift
pat=${AB_PAT:-"k_raster_fwd<K|k_sil_bwd|k_raster_fwd<1|k_tex_bwd|sum of"}
for rep in 1 2; do
  for v in "$@"; do
    if [ "$v" = "-" ]; then lib=acfm_video_3d_reconstruction_amd/libacfm_hip.so; else lib=acfm_video_3d_reconstruction_amd/libacfm_hip_$v.so; fi
    echo "== $v (round $rep)"
    ACFM_LIB=$PWD/$lib python tools/kbench.py $args 2>&1 | grep -E "$pat"
  done
done
