"""bench.py host logic (no GPU): the multi-GPU launcher and the roofline
arithmetic of SURVEY §8(d)."""
import os
import subprocess
import sys

import pytest

import bench


def test_launcher_command_runs_torchrun_as_child():
    cmd = bench.launcher_command(["--gpus", "2", "--steps", "3"], 2, port=29511)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=2" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and "--master-port=29511" in cmd
    assert cmd[cmd.index("--master-port=29511") + 1] == os.path.abspath(bench.__file__)
    assert cmd[-4:] == ["--gpus", "2", "--steps", "3"]


def test_gpus_flag_spawns_ranks_without_touching_the_gpu(monkeypatch):
    """`bench.py --gpus 4` outside torchrun starts the rank launcher as a
    subprocess and exits with its return code (never an exec)."""
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2"])
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: pytest.fail("touched the GPU"))
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    assert "--nproc-per-node=4" in seen["cmd"] and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_encode_bytes_per_image_matches_survey():
    # 3,591,168 B per 512^2 image, 713,472 B per 224^2 image
    assert bench.encode_bytes_per_image(512, 512, 3072, 14, 3072, 1) == 3591168
    assert bench.encode_bytes_per_image(224, 224, 768, 14, 3072, 4) == 713472


def _packed(rows, s=16, ncb=14, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return {"codes": torch.randint(0, 2 ** 14, (rows, s, ncb), generator=g),
            "positions": torch.randint(0, 32, (rows, s, 2), generator=g),
            "channels": torch.randint(0, 3, (rows, s), generator=g),
            "image_ids": torch.arange(rows)[:, None].expand(rows, s).contiguous(),
            "key_pad_mask": torch.rand(rows, s, generator=g) < 0.25}


@pytest.mark.parametrize("rows", [5, 300])
def test_dump_outputs_writes_a_fixed_sample_exactly(tmp_path, rows):
    """--dump-outputs: float32 / float64 .npy files; the sampled rows are the
    same from call to call, hold the packed values exactly, and the per-row
    sums cover every row."""
    import numpy as np
    out = _packed(rows)
    bench.dump_outputs(out, str(tmp_path / "a"), 0)
    bench.dump_outputs(out, str(tmp_path / "b"), 0)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(f"{k}.npy" for k in ("codes", "positions", "channels", "image_ids", "key_pad_mask",
                                                  "sample_rows", "codes_row_sum", "tokens_per_row"))
    arrays = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert arrays[n[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(arrays[n[:-4]], np.load(tmp_path / "b" / n))
    sel = arrays["sample_rows"].astype(np.int64)
    assert len(sel) == min(rows, bench.DUMP_ROWS) and len(set(sel.tolist())) == len(sel) and sel.max() < rows
    for k in ("codes", "positions", "channels", "image_ids", "key_pad_mask"):
        assert np.array_equal(arrays[k].astype(np.int64), out[k].numpy()[sel].astype(np.int64))
    assert np.array_equal(arrays["codes_row_sum"], out["codes"].sum(dim=(1, 2)).numpy().astype(np.float64))
    assert np.array_equal(arrays["tokens_per_row"], (~out["key_pad_mask"]).sum(dim=1).numpy().astype(np.float64))
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20


def test_dump_outputs_of_the_headline_geometry_fits_64_mb():
    """1024 rows x 3072 tokens x 14 codebooks: the sample's bytes, from the shapes."""
    r, s, ncb = bench.DUMP_ROWS, 3072, 14
    sample = 4 * r * s * (ncb + 2 + 1 + 1 + 1)
    assert sample + 8 * (r + 2 * 1024) <= 64 * 10 ** 6


def test_other_rank_dumps_beside_rank_0(tmp_path):
    bench.dump_outputs(_packed(3), str(tmp_path), 2)
    assert "codes.rank2.npy" in os.listdir(tmp_path)
