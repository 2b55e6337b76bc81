"""Multi-step rollout inference of the AVERAGED weights of a run trained with --ema_decay: harness/test_multistep.py's tool (same flags,
same cases, same metrics, same sharding over the ranks of a ``torch.distributed`` launch) on ``model_ema.pt`` of the best checkpoint
instead of ``model.pt``.  It writes ``multistep_metrics_ema.json``, so the trained model's ``multistep_metrics.json`` stays beside it.

    python -m cfdbench_amd.harness.multistep_ema --model fno --data dam_prop_bc_geo --infer_steps 200

A run that kept no averaged weights is an error that names the missing file, raised before the data is read or a GPU is touched.
"""
from __future__ import annotations

from pathlib import Path

from .args import Args, is_args_valid
from .autoregressive import init_model
from .common import best_ckpt_file, dump_json, get_output_dir, load_ckpt
from .test_multistep import infer, prepare_cases, shard_cases


def main(argv=None):
    from .data import get_auto_dataset
    from .dist_util import init_distributed
    args = Args().parse_args(argv)
    is_args_valid(args)
    output_dir = get_output_dir(args, is_auto=True)
    ckpt = best_ckpt_file(output_dir, use_ema=True)  # (first: nothing to roll out without it)
    rank, world = init_distributed()  # one process per GPU; a plain start stays single-process
    if rank == 0:
        print(args)
    _, _, test_data = get_auto_dataset(data_dir=Path(args.data_dir), data_name=args.data_name, delta_time=args.delta_time,
                                       norm_props=bool(args.norm_props), norm_bc=bool(args.norm_bc), load_splits=["test"])
    n_cases = len(test_data.all_features)
    feats, cps = prepare_cases(test_data, args.infer_steps, only=set(shard_cases(n_cases, rank, world)))
    model = init_model(args).cuda()
    load_ckpt(model, ckpt)  # every rank reads rank 0's checkpoint tree: identical replicas, no broadcast needed
    all_metrics = infer(model, feats, cps, args.infer_steps, dtype=args.dtype, n_total_cases=n_cases)
    if rank == 0:
        dump_json(all_metrics, output_dir / "multistep_metrics_ema.json")
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
