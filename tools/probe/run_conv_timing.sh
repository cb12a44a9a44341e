# development: per-workgroup phase timing of the fp32 conv kernel (conv.hip built with -DY3_TIMING)
P=tools/probe/conv_timing
for shape in "8 52 128 256 3" "8 52 256 128 1" "8 26 512 256 1" "8 13 1024 512 1"; do
  echo "=== $shape"; $P $shape || exit 1
done
