"""CPU-side checks of the drop-in boundary: the C-ABI library is built in-tree, loads,
exports every symbol include/tt_hotpath.h declares, the ctypes table covers exactly those
symbols, and the product path refuses to run without a GPU (no CPU fallback)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "tt_hotpath.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from two_tower_models_amd import _native as N
    lib = N.load()
    names = header_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/tt_hotpath.h but not exported"
    assert sorted(N.SIGNATURES) == names
    assert lib.tt_abi_version() == N.ABI_VERSION


def test_argument_validation_needs_no_gpu():
    from two_tower_models_amd import _native as N
    lib = N.load()
    assert lib.tt_gather_rows(None, 1, 1, None, 1, None, 1, None, None) == -1  # TT_E_BADARG
    assert b"null pointer" in lib.tt_last_error_string()
    assert lib.tt_gemm_workspace_bytes(N.TT_GEMM_TN, 128, 384, 409600) > 0
    assert lib.tt_inbatch_ce_workspace_bytes(8192, 8192, 128) > 0
    assert lib.tt_inbatch_ce_workspace_bytes(8192, 8192, 256) >= 8192 * 8192 * 4  # D > 128: logits materialised
    # the fused tower: D, F, hidden, d_out, third-block width E
    assert [lib.tt_tower_supported(*a) for a in ((128, 8, 256, 128, 0), (128, 8, 256, 128, 256), (128, 8, 256, 128, 64),
                                                 (96, 8, 256, 96, 0))] == [1, 1, 0, 0]
    # one or two sides per call, two without a third block; refused before any HIP call (B = 64, D = 128, hidden = 256)
    for call, side in ((lambda s, n, E: lib.tt_tower_fwd(s, n, 64, 128, 256, E, None, None), N.TowerFwdSide),
                       (lambda s, n, E: lib.tt_tower_bwd_data(s, n, 64, 128, 256, E, None), N.TowerBwdSide),
                       (lambda s, n, E: lib.tt_tower_bwd_weights(s, n, 64, 128, 256, E, None), N.TowerWgradSide)):
        assert call(None, 1, 0) == N.TT_E_BADARG
        assert call((side * 3)(), 0, 0) == N.TT_E_BADARG and call((side * 3)(), 3, 0) == N.TT_E_BADARG
        assert call((side * 2)(), 2, 256) == N.TT_E_UNSUPPORTED
        assert call(side(), 1, 0) == N.TT_E_BADARG and b"null pointer" in lib.tt_last_error_string()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU refusal")
def test_no_cpu_fallback():
    import two_tower_models_amd as A
    mips = A.BaselineMIPSModule(16, 8)
    m = A.TwoTowerBaseRetrieval(4, 10, 8, 4, 10, 8, 4, [1.0], mips)
    B = 4
    args = (torch.zeros(B, dtype=torch.long), torch.zeros(B, 4), torch.zeros(B, 2, dtype=torch.long),
            torch.zeros(B, dtype=torch.long), torch.zeros(B, 4), torch.zeros(B, dtype=torch.long), torch.ones(B, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.train_forward(*args)


def test_module_surface_matches_reference_names():
    """Constructor keywords, method names and state_dict keys of the reference API."""
    import inspect
    import two_tower_models_amd as A
    sig = inspect.signature(A.TwoTowerBaseRetrieval.__init__)
    assert list(sig.parameters)[1:] == ["num_items", "user_id_hash_size", "user_id_embedding_dim",
                                        "user_features_size", "item_id_hash_size", "item_id_embedding_dim",
                                        "item_features_size", "user_value_weights", "mips_module"]
    for meth in ("get_user_embedding", "process_user_features", "compute_user_embedding",
                 "compute_item_embeddings", "forward", "debias_net_user_value", "compute_training_loss",
                 "train_forward"):
        assert callable(getattr(A.TwoTowerBaseRetrieval, meth))
    mips = A.BaselineMIPSModule(corpus_size=16, embedding_dim=8)
    assert mips.corpus_size == 16 and mips.corpus.shape == (16, 8) and len(mips.state_dict()) == 0
    m = A.TwoTowerWithDebiasing(4, 10, 8, 4, 6, 10, 8, 4, [1.0], mips)
    keys = set(m.state_dict())
    for k in ("user_id_embedding_arch.weight", "user_features_arch.0.weight", "user_features_arch.2.bias",
              "user_tower_arch.weight", "item_id_embedding_arch.weight", "item_tower_arch.bias",
              "user_history_encoder.multihead_attn_layers.2.in_proj_weight",
              "user_history_encoder.multihead_attn_layers.0.out_proj.bias",
              "position_bias_net_user_value.weight", "user_debias_net_user_value.0.weight"):
        assert k in keys, k
    assert m.user_tower_arch.weight.shape == (8, 2 * 8 + 2 * 8)
    # the two single-term siblings: same constructor keywords, one extra parameter tensor (pair) each
    kw = ["num_items", "user_id_hash_size", "user_id_embedding_dim", "user_features_size", "user_history_seqlen",
          "item_id_hash_size", "item_id_embedding_dim", "item_features_size", "user_value_weights", "mips_module"]
    for cls, extra in ((A.TwoTowerWithPositionDebiasedWeights, {"position_bias_net_user_value.weight": (100, 1)}),
                       (A.TwoTowerWithUserDebiasedWeights, {"user_debias_net_user_value.0.weight": (1, 8),
                                                            "user_debias_net_user_value.0.bias": (1,)})):
        assert list(inspect.signature(cls.__init__).parameters)[1:] == kw
        sd = cls(4, 10, 8, 4, 6, 10, 8, 4, [1.0], mips).state_dict()
        assert set(sd) - set(A.TwoTowerWithUserHistoryEncoder(4, 10, 8, 4, 6, 10, 8, 4, [1.0], mips).state_dict()) == set(extra)
        assert all(tuple(sd[k].shape) == shp for k, shp in extra.items())
    enc = A.UserHistoryEncoder(8, 6, 2, 1, True)
    assert enc.get_output_dim() == 16 and enc.positional_embeddings.shape == (6, 8)


def test_bench_roofline_traffic_key_resolves(tmp_path):
    """bench.py's roofline.traffic comes from profiles/pmc_traffic.json: the key the default run looks up must exist
    (round 3 shipped a flat record and the driver's line carried `"traffic": null`), in the keyed and the flat form."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    path = os.path.join(root, "profiles", "pmc_traffic.json")
    got = bench.pmc_traffic_bytes(path, "P", 1)
    alg = bench.algorithmic_sweep_bytes(bench.WORKLOADS["P"], 1)
    assert got is not None and 0.98 * alg < got < 1.10 * alg, (got, alg)
    assert bench.pmc_traffic_bytes(path, "C2", 1) is None  # no measurement committed for that workload: null, not a wrong number
    flat = str(tmp_path / "pmc_flat_test.json")
    json.dump(json.load(open(path))["P_gpus1"], open(flat, "w"))
    assert bench.pmc_traffic_bytes(flat, "P", 1) == got


def test_bench_dump_outputs_sample_and_limit(tmp_path):
    """`bench.py --dump-outputs`: a table's sample is the last step's looked-up rows plus seeded uniform rows, the same on
    every call, restricted to the block a row-sharded table holds; the arrays land as float32 / float64 .npy files and more
    than 64 MB in all is refused."""
    import importlib.util

    import numpy as np

    from two_tower_models_amd import parallel
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    whole = torch.nn.Parameter(torch.zeros(100_000, 4))
    ids = [torch.tensor([5, 99_999, 5, 70_000])]
    rows, local = bench._table_rows_sample(whole, ids)
    again, _ = bench._table_rows_sample(whole, ids)
    assert torch.equal(rows, again) and torch.equal(rows, local) and torch.equal(rows, torch.unique(rows))
    assert {5, 99_999, 70_000} <= set(rows.tolist()) and len(rows) <= 4 + bench.DUMP_TABLE_ROWS
    block = torch.nn.Parameter(torch.zeros(50_000, 4))
    block._tt_shard = parallel.RowShard(100_000, 4, 2, 1)  # rows [50 000, 100 000)
    brows, blocal = bench._table_rows_sample(block, ids)
    assert torch.equal(brows, rows[rows >= 50_000]) and torch.equal(blocal, brows - 50_000)
    bench.dump_outputs(str(tmp_path / "d"), {"loss": torch.tensor(0.5), "ids": torch.arange(3),
                                             "w": torch.ones(2, 2, dtype=torch.bfloat16)})
    got = {n: np.load(tmp_path / "d" / n) for n in sorted(os.listdir(tmp_path / "d"))}
    assert {n: a.dtype for n, a in got.items()} == {"ids.npy": np.float64, "loss.npy": np.float32, "w.npy": np.float32}
    assert got["ids.npy"].tolist() == [0.0, 1.0, 2.0] and float(got["loss.npy"]) == 0.5
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": torch.zeros(17 << 20)})
    assert not os.path.exists(tmp_path / "big")


def test_reference_package_name_resolves_to_this_implementation():
    """`from src.<module> import <Class>` (the reference's layout, ref:tests/conftest.py:1-6) gives this package's classes."""
    import two_tower_models_amd as A
    from src.baseline_mips_module import BaselineMIPSModule
    from src.two_tower_base_retrieval import TwoTowerBaseRetrieval
    from src.two_tower_with_debiasing import TwoTowerWithDebiasing
    from src.two_tower_with_user_history_encoder import TwoTowerWithUserHistoryEncoder
    from src.user_history_encoder import UserHistoryEncoder
    assert TwoTowerBaseRetrieval is A.TwoTowerBaseRetrieval and BaselineMIPSModule is A.BaselineMIPSModule
    assert TwoTowerWithDebiasing is A.TwoTowerWithDebiasing and UserHistoryEncoder is A.UserHistoryEncoder
    assert TwoTowerWithUserHistoryEncoder is A.TwoTowerWithUserHistoryEncoder


def test_mips_corpus_assignment_drops_the_split_fp16_copy():
    """the split-fp16 copy belongs to ONE corpus tensor; a key of (pointer, version, shape) cannot tell a
    re-allocated corpus at the same address from the old one, so every assignment of `corpus` invalidates it."""
    import torch

    from two_tower_models_amd.baseline_mips_module import BaselineMIPSModule
    m = BaselineMIPSModule(16, 128)
    assert m.state_dict() == {} and tuple(m.corpus.shape) == (16, 128)  # still a plain tensor attribute (ref :29-30)
    for assign in (lambda: setattr(m, "corpus", torch.zeros(16, 128)), lambda: m.set_corpus(torch.ones(8, 128)),
                   lambda: m.use_bf16_storage(), lambda: m.to(torch.device("cpu"))):
        m._split16, m._split16_key = object(), ("stale",)
        assign()
        assert m._split16 is None and m._split16_key is None
    assert m.corpus.dtype == torch.bfloat16 and m.corpus_size == 8
