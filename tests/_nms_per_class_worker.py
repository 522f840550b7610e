"""Worker for tests/test_nms_per_class_cpu.py: world-2 gloo all-gather of padded box lists sized by a per-class engine's
capacity (cls_cnt * max_out rows per image)."""
import os
import sys


def main(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "bayesian-yolov3_amd"))
    import torch
    import torch.distributed as dist
    from byolo import Engine, NMS_PER_CLASS, dist as bdist
    bdist.init(backend="gloo")
    C, max_out, D = 3, 4, 9
    eng = Engine((64, 64, 3), C, nms_mode=NMS_PER_CLASS, max_out=max_out)
    cap = eng.out_cap                                 # what Inference sizes its slots by
    n_glob = 3                                        # blocks of 2 and 1 images, padded to 2
    lo, hi = bdist.shard_range(n_glob, rank, world)
    bl = bdist.padded_block(n_glob, world)
    rows = torch.zeros((bl, cap, D)); kept = torch.full((bl, cap), -1, dtype=torch.int32)
    count = torch.zeros((bl, 2), dtype=torch.int32)
    for j in range(hi - lo):
        g = lo + j
        k = cap - g                                   # image 0 fills all C * max_out rows: beyond what two classes could hold
        rows[j, :k] = 100.0 * g + torch.arange(D, dtype=torch.float32)
        kept[j, :k] = torch.arange(k, dtype=torch.int32) + 1000 * g
        count[j, 0] = k; count[j, 1] = min(k, max_out)
    g_rows, g_kept, g_count = bdist.allgather_boxes(rows, kept, count, world)
    u_rows, u_kept = bdist.unpack_global(g_rows, g_kept, g_count, n_glob, world)
    torch.save({"cap": cap, "g_rows_shape": tuple(g_rows.shape), "g_kept_shape": tuple(g_kept.shape), "u_rows": u_rows, "u_kept": u_kept},
               os.path.join(out_dir, "rank%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
