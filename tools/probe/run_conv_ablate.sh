# development: K-loop cost of the fp32 conv kernel with parts of the step ablated (tools/probe/conv_timing, Y3_ABL), planned tiles
P=tools/probe/conv_timing
for abl in 0 1 2 3 4 7; do
  echo "=== 1x1 256->128 M=21632, ABL=$abl"; Y3_ABL=$abl $P 8 52 256 128 1 || exit 1
done
for abl in 0 1 2 3 4 7; do
  echo "=== 3x3 128->128 M=32768, ABL=$abl"; Y3_ABL=$abl $P 2 128 128 128 3 || exit 1
done
