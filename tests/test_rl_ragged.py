"""Ragged RL rollouts on the CPU (fp32): left-aligned prompts of different
lengths, EOS stop, per-row response windows in the PPO trainer, config
plumbing, and a tensor-parallel actor over gloo."""

import os

import pytest
import torch
import torch.multiprocessing as mp

from conftest import free_port
from dlrover_wuqiong_amd.atorch.rl.config import PPOConfig
from dlrover_wuqiong_amd.atorch.rl.engine import ModelEngine, ValueModel
from dlrover_wuqiong_amd.atorch.rl.hybrid_engine import HybridEngine
from dlrover_wuqiong_amd.atorch.rl.ppo_utils import logprobs_of_labels
from dlrover_wuqiong_amd.atorch.rl.rl_config import AtorchRLConfig, LastTokenScorer, PromptDataset
from dlrover_wuqiong_amd.atorch.rl.trainer import PPOTrainer
from dlrover_wuqiong_amd.models.llama import Llama, LlamaConfig

LENS = [3, 9, 1, 6]
PMAX, NEW, PAD = 9, 6, 0


def _model(seed=0):
    torch.manual_seed(seed)
    return Llama(LlamaConfig.named("llama-tiny")).eval()


def _prompts(fill_seed=1):
    """Left-aligned [4, 9] prompts; the cells after each prompt hold garbage
    drawn from ``fill_seed`` (the real tokens do not depend on it)."""
    real = torch.randint(1, 1024, (len(LENS), PMAX), generator=torch.Generator().manual_seed(7))
    junk = torch.randint(1, 1024, (len(LENS), PMAX), generator=torch.Generator().manual_seed(fill_seed))
    keep = torch.arange(PMAX)[None] < torch.tensor(LENS)[:, None]
    return torch.where(keep, real, junk), torch.tensor(LENS)


@pytest.fixture(scope="module")
def dense():
    """The oracle: every row generated alone, unpadded, by the dense path."""
    m = _model()
    p, _ = _prompts()
    eng = HybridEngine(m, 4, 32)
    return m, [eng.generate(p[b:b + 1, :n], NEW, temperature=0)[0] for b, n in enumerate(LENS)]


def _expected(row, n, eos):
    """prompt | response cut after its first ``eos`` | pad, and the response length."""
    out = torch.full((PMAX + NEW,), PAD, dtype=torch.long)
    resp = row[n:].tolist()
    if eos is not None and eos in resp:
        resp = resp[:resp.index(eos) + 1]
    out[:n] = row[:n]
    out[n:n + len(resp)] = torch.tensor(resp)
    return out, len(resp)


def test_left_align_inverts_left_padding():
    raw = [[5, 6, 7], list(range(10, 22)), [9], [1, 2, 3, 4, 5, 6], list(range(30, 38))]
    ds = PromptDataset(raw, max_prompt_length=8, pad_token_id=99)
    assert ds.prompt_lens.tolist() == [3, 8, 1, 6, 8]
    assert ds.lens_of([2, 0]).tolist() == [1, 3] and int(ds.lens_of(1)) == 8
    assert ds[0].tolist() == [99] * 5 + [5, 6, 7]  # the default output is still left-padded
    batch = next(iter(ds.create_loader(5)))
    assert torch.equal(batch, ds.gen_prompts)
    al = ds.left_align(batch, ds.prompt_lens)
    for row, p, n in zip(al, raw, ds.prompt_lens.tolist()):
        assert row[:n].tolist() == p[-8:] and row[n:].tolist() == [99] * (8 - n)


def test_ragged_greedy_matches_rows_generated_alone(dense):
    from dlrover_wuqiong_amd.atorch.rl.trainer import sample_ragged

    m, rows = dense
    p, lens = _prompts()
    seq, pl, rl = HybridEngine(m, 4, 32).generate_ragged(p, lens, NEW, temperature=0, pad_token_id=PAD)
    assert seq.shape == (4, PMAX + NEW) and pl.tolist() == LENS and rl.tolist() == [NEW] * 4
    for b, n in enumerate(LENS):
        assert torch.equal(seq[b], _expected(rows[b], n, None)[0]), b
    seq2, _, rl2 = sample_ragged(m, p, lens, NEW, temperature=0, pad_token_id=PAD)
    assert torch.equal(seq2, seq) and torch.equal(rl2, rl)


def test_cells_after_a_prompt_change_nothing(dense):
    m, _ = dense
    eng = HybridEngine(m, 4, 32)
    a = eng.generate_ragged(*_prompts(1), NEW, temperature=0)[0]
    b = eng.generate_ragged(*_prompts(2), NEW, temperature=0)[0]
    assert not torch.equal(_prompts(1)[0], _prompts(2)[0]) and torch.equal(a, b)


def test_eos_cuts_each_row_and_stops_the_rollout(dense):
    from dlrover_wuqiong_amd.atorch.rl.trainer import sample_ragged

    m, rows = dense
    p, lens = _prompts()
    eos = int(rows[1][LENS[1] + 2])  # row 1 emits it as its third response token
    want = [_expected(rows[b], n, eos) for b, n in enumerate(LENS)]
    assert want[1][1] <= 3
    eng = HybridEngine(m, 4, 32)
    for interval in (1, 8):
        seq, _, rl = eng.generate_ragged(p, lens, NEW, temperature=0, eos_token_id=eos, pad_token_id=PAD,
                                         eos_check_interval=interval)
        assert rl.tolist() == [w[1] for w in want]
        for b in range(4):
            assert torch.equal(seq[b], want[b][0]), (interval, b)
    seq2, _, rl2 = sample_ragged(m, p, lens, NEW, temperature=0, eos_token_id=eos, pad_token_id=PAD)
    assert torch.equal(seq2, seq) and torch.equal(rl2, rl)

    # an EOS every row reaches: identical prompts, EOS = their second response token
    one = p[1:2].expand(4, PMAX).contiguous()
    full = torch.full((4,), PMAX)
    eos_all = int(rows[1][PMAX + 1])
    n_first = rows[1][PMAX:].tolist().index(eos_all) + 1
    calls = []
    fwd = eng._forward
    eng._forward = lambda *a, **k: (calls.append(1), fwd(*a, **k))[1]
    long_new = 12
    seq, _, rl = eng.generate_ragged(one, full, long_new, temperature=0, eos_token_id=eos_all, pad_token_id=PAD,
                                     eos_check_interval=1)
    assert rl.tolist() == [n_first] * 4 and len(calls) < long_new
    assert (seq[:, PMAX + n_first:] == PAD).all()


class _Reward(torch.nn.Module):
    """Depends on every real token of the row and on nothing else."""

    def forward(self, ids, lengths=None):
        if lengths is None:
            lengths = torch.full((ids.shape[0],), ids.shape[1], device=ids.device)
        keep = torch.arange(ids.shape[1], device=ids.device)[None] < lengths[:, None]
        return ((ids % 11) * keep).sum(1).float() / lengths


def _trainer(pad, eos, seed=0):
    torch.manual_seed(seed)
    cfg = LlamaConfig.named("llama-tiny")
    actor, ref = Llama(cfg), Llama(cfg)
    critic = ValueModel(Llama(cfg), cfg.vocab_size)
    eng = ModelEngine(actor, critic, ref, _Reward(), actor_lr=1e-4, critic_lr=1e-4)
    pc = PPOConfig(max_new_tokens=NEW, rollout_batch_size=4, mini_batch_size=4, ppo_epochs=1, temperature=0.0,
                   eos_token_id=eos, pad_token_id=pad, eos_check_interval=2)
    return PPOTrainer(eng, None, pc), eng


def _left_padded(pad):
    p, lens = _prompts()
    out = torch.full_like(p, pad)
    for b, n in enumerate(LENS):
        out[b, PMAX - n:] = p[b, :n]
    return out, lens


def _eos_for_trainer():
    tr, eng = _trainer(PAD, None)
    eng.eval()
    p, lens = _prompts()
    seq = HybridEngine(eng.actor, 4, 32).generate_ragged(p, lens, NEW, temperature=0)[0]
    return int(seq[1, LENS[1] + 2])


def test_make_experience_windows_mask_and_scores():
    eos = _eos_for_trainer()
    exps, losses = [], []
    for pad in (0, 777):
        tr, eng = _trainer(pad, eos)
        eng.eval()
        tr.make_experience(*_left_padded(pad))
        exps.append(tr.buffer.items[0])
        eng.train()
        losses.append(tr.rl_training()["loss/total"])
    e = exps[0]
    R = NEW
    resp_lens = e.mask.sum(1).long()
    assert e.sequences.shape == (4, PMAX + R) and e.prompt_lens.tolist() == LENS
    assert int(resp_lens[1]) <= 3 and int(resp_lens.min()) >= 1  # row 1 stopped at its EOS
    assert torch.equal(e.mask, (torch.arange(R)[None] < resp_lens[:, None]).float())
    tr, eng = _trainer(0, eos)
    eng.eval()
    with torch.no_grad():
        for b, n in enumerate(LENS):
            r = int(resp_lens[b])
            row = e.sequences[b:b + 1, :n + r]  # the row alone at its true length
            assert (e.sequences[b, n + r:] == 0).all()
            if r < R:
                assert int(row[0, -1]) == eos
            lp = logprobs_of_labels(eng.actor(row)[:, n - 1:-1], row[:, n:])[0]
            torch.testing.assert_close(e.logprobs[b, :r], lp, atol=1e-5, rtol=0)
            assert (e.logprobs[b, r:] == 0).all()
            torch.testing.assert_close(e.scores[b], _Reward()(row, torch.tensor([n + r]))[0], atol=1e-6, rtol=0)
    # nothing but the pad cells of the sequences knows the pad token
    o = exps[1]
    real = torch.arange(PMAX + R)[None] < (e.prompt_lens + resp_lens)[:, None]
    assert torch.equal(torch.where(real, e.sequences, 0), torch.where(real, o.sequences, 0))
    assert (o.sequences[~real] == 777).all()
    for k in ("logprobs", "values", "advantages", "returns", "mask", "scores", "prompt_lens"):
        assert torch.equal(getattr(e, k), getattr(o, k)), k
    assert losses[0] == losses[1]


def test_last_token_scorer_reads_the_last_real_token():
    class Trunk(torch.nn.Module):
        def forward(self, ids):
            return ids.float()  # [B, S] "values"

    ids = torch.tensor([[4, 5, 6, 0, 0], [7, 8, 9, 10, 11]])
    s = LastTokenScorer(Trunk())
    assert s(ids).tolist() == [0.0, 11.0]
    assert s(ids, lengths=torch.tensor([3, 5])).tolist() == [6.0, 11.0]


def _rl_config(gen_kwargs, data=None):
    role = {"model_cls": "dlrover_wuqiong_amd.models.llama.Llama", "model_params": {"config": "llama-tiny"}}
    return AtorchRLConfig.from_dict({
        "model": {"actor": dict(role), "critic": dict(role), "reward_model": dict(role)},
        "generation": {"batch_size": 4, "gen_experience_kwargs": dict({"max_new_tokens": 4}, **gen_kwargs)},
        "data": data or {}})


def test_config_carries_eos_and_pad():
    ppo = _rl_config({"eos_token_id": 2, "pad_token_id": 3}).to_ppo_config()
    assert (ppo.eos_token_id, ppo.pad_token_id, ppo.fused_kv_append, ppo.eos_check_interval) == (2, 3, False, 8)
    ppo = _rl_config({}, {"pad_token_id": 5}).to_ppo_config()
    assert (ppo.eos_token_id, ppo.pad_token_id) == (None, 5)
    # neither lengths nor EOS: the dense rollout, all-ones mask
    tr, eng = _trainer(0, None)
    eng.eval()
    tr.make_experience(torch.randint(1, 1024, (4, 5)))
    e = tr.buffer.items[0]
    assert e.sequences.shape == (4, 5 + NEW) and e.prompt_lens is None and bool((e.mask == 1).all())


def test_train_passes_dataset_lengths_when_eos_is_set():
    eos = _eos_for_trainer()
    tr, eng = _trainer(0, eos)
    p, _ = _prompts()
    tr.dataset = PromptDataset([p[b, :n].tolist() for b, n in enumerate(LENS)], PMAX, pad_token_id=0)
    seen = []
    post = tr.post_rl_training_hook
    tr.post_rl_training_hook = lambda: (seen.append(tr.buffer.items[0]), post())
    tr.train(1)
    assert sorted(seen[0].prompt_lens.tolist()) == sorted(LENS)


def _tp_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dlrover_wuqiong_amd.models.llama import shard_llama_state_dict

        full = _model()
        cfg = full.cfg
        p, lens = _prompts()
        ref = HybridEngine(full, 4, 32).generate_ragged(p, lens, NEW, temperature=0)
        eos = int(ref[0][1, LENS[1] + 2])
        ref = HybridEngine(full, 4, 32).generate_ragged(p, lens, NEW, temperature=0, eos_token_id=eos)
        tp = Llama(cfg, tp_group=dist.group.WORLD).eval()
        tp.load_state_dict(shard_llama_state_dict(full.state_dict(), cfg, rank, world))
        eng = HybridEngine(tp, 4, 32)
        out = eng.generate_ragged(p, lens, NEW, temperature=0, eos_token_id=eos, eos_check_interval=2)
        # sampled: both ranks must emit the same tokens from different generators
        out2 = eng.generate_ragged(p, lens, NEW, temperature=1.0, eos_token_id=eos,
                                   generator=torch.Generator().manual_seed(rank))[0]
        both = [torch.zeros_like(out2) for _ in range(world)]
        dist.all_gather(both, out2)
        q.put((rank, torch.equal(out[0], ref[0]) and torch.equal(out[2], ref[2]) and torch.equal(both[0], both[1])))
    except Exception as e:  # pragma: no cover
        import traceback

        traceback.print_exc()
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_tensor_parallel_actor_ragged_generation():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    ps = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=180) for _ in ps)
    for p in ps:
        p.join(30)
    assert all(r[1] is True for r in res), res
