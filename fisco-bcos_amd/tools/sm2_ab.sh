# A/B of SM2 trio-kernel variants on c2sm2 (10k SM2 txs): the default library and the round-3 schedule
# without the low-window chains (BCOSGPU_SM2_SPLIT=0), alternated twice.
#   -> gpurun_out/sm2ab_<tag>_<k>.json (bench lines)
set -o pipefail
A="--workload c2sm2 --steps 3000 --warmup 20 --legs= --no-cpu-baseline --no-merkle --no-extras --no-hashes --devset none --detail-out="
for k in 1 2; do
  for tag in default split0; do
    envs="BCOSGPU_X=1"
    case $tag in split0) envs="BCOSGPU_SM2_SPLIT=0";; esac
    env $envs timeout -k 10 200 python3 -u bench.py $A > gpurun_out/sm2ab_${tag}_$k.json 2> gpurun_out/sm2ab_${tag}_$k.err
    rc=$?
    [ $rc -eq 0 ] || { echo "$tag failed"; tail -3 gpurun_out/sm2ab_${tag}_$k.err; exit 1; }
    python3 -c "
import json; l=json.loads(open('gpurun_out/sm2ab_${tag}_$k.json').read().strip().splitlines()[-1])
print('$tag $k', round(l['ms_per_step'], 4), l['roofline'].get('kernel_ms'))"
  done
done
