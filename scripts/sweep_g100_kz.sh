cd "$(dirname "$0")/.." || exit 1; export TMPDIR=/tmp; O=${OUT:-bench_out}/sw; mkdir -p $O
for r in 1 2; do
for kz in 0 1 2 3 5; do
  timeout -k 10 120 python bench.py --grid-nodes 100 --steps 2000 --warmup 20 --full --no-cpu --kz $kz --prewarm-s 0.2 > $O/kz$kz.json 2>>$O/err.log || exit 1
  python3 -c "import json;d=json.load(open('$O/kz$kz.json'));print('kz $kz', d['value'], round(d['ms_per_step']*1e3,1), d['roofline']['stages_ms'])"
done
done
