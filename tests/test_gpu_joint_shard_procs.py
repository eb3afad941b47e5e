"""tpe.suggest(..., joint_shard=(rank, world)) end to end (DESIGN.md "Sharded
joint stage"): two processes (gloo, both on the one GPU) each score their half
of every joint stage's candidates and exchange the winner records; one nccl rank
with the exchange forced on sends its records through RCCL.  The contract is
byte equality with the call without the keyword: every value of every document
compares == (no tolerance), on every rank."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

N_CAND = 2 * 1024 + 37          # the two ranks' parts meet inside the second chunk
N_HIST = 60
BRANCH_KW = dict(joint=True, joint_discrete=True, joint_quantized=True, joint_branches=True,
                 joint_branches_mixed=True)


def _history(space, seed):
    """N_HIST prior draws of ``space`` with a seeded loss."""
    from hyperopt_amd import base, rand
    domain = base.Domain(lambda d: 0.0, space)
    trials = base.Trials()
    rs = np.random.RandomState(seed)
    for tid in range(N_HIST):
        docs = rand.suggest([tid], domain, trials, int(rs.randint(2 ** 31 - 1)))
        docs[0]['state'] = base.JOB_STATE_DONE
        docs[0]['result'] = {'status': 'ok', 'loss': float(rs.uniform())}
        trials.insert_trial_docs(docs)
    trials.refresh()
    return domain, trials


def _cases():
    """(name, domain, trials, new ids, seed, keywords): a flat space of 4
    continuous labels, a choice and a quniform joined in one quantised group;
    bench.py's tree with all five keywords and 3 batched ids (no root group: the
    segmented branch stage alone; bench.rf_loss steers the gate to the rf
    branch, whose group holds a discrete and a quantised label); 20 uniform
    labels in one wide group."""
    import bench
    from hyperopt_amd import hp
    flat = {'x': hp.uniform('x', -10, 10), 'y': hp.loguniform('y', -3, 1), 'z': hp.normal('z', 0, 2),
            'w': hp.lognormal('w', 0, 1), 'c': hp.choice('c', ['a', 'b', 'c']), 'q': hp.quniform('q', 0, 10, 1)}
    wide = dict(('u%02d' % i, hp.uniform('u%02d' % i, -1 - i, 2 + i)) for i in range(20))
    out = [('flat',) + _history(flat, 1) + ([N_HIST, N_HIST + 5], 31,
                                            dict(joint=True, joint_discrete=True, joint_quantized=True)),
           ('tree',) + tuple(bench.make_history(N_HIST, 0, bench.rf_loss)) + ([N_HIST, N_HIST + 1, N_HIST + 2], 32, BRANCH_KW),
           ('wide',) + _history(wide, 3) + ([N_HIST], 33, dict(joint=True, joint_wide=True))]
    return out


def _plain(docs):
    """Per document {label: [type name, the float's hex]}: == on every value, and
    the types the unsharded suggest gives."""
    return [{k: [[type(x).__name__, float(x).hex()] for x in v] for k, v in sorted(d['misc']['vals'].items())}
            for d in docs]


def _suggest_all(**kw):
    from hyperopt_amd import tpe
    return dict((name, _plain(tpe.suggest(ids, domain, trials, seed, n_EI_candidates=N_CAND, **dict(jkw, **kw))))
                for name, domain, trials, ids, seed, jkw in _cases())


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        q.put((rank, _suggest_all(joint_shard=(rank, world)), None))
    except Exception:               # report, do not hang the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_return_the_unsharded_documents():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    ref = _suggest_all()                             # the unsharded suggest, beside the two ranks
    got = {}
    for _ in procs:
        rank, out, err = q.get(timeout=240)
        assert err is None, (rank, err)
        got[rank] = out
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(ref) == ['flat', 'tree', 'wide']
    joined = dict(flat=['c', 'q', 'w', 'x', 'y', 'z'], wide=['u%02d' % i for i in range(20)])
    for name in ref:
        assert got[0][name] == got[1][name], name    # every rank holds the whole result
        assert got[0][name] == ref[name], name       # ... the unsharded one, value for value
        for doc in ref[name]:
            assert all(len(doc[k]) == 1 for k in joined.get(name, []))


def _nccl_worker(port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        from hyperopt_amd import _native as N, dist as D
        from hyperopt_amd.engine import Engine, get_engine
        ref = _suggest_all()
        eng = get_engine()
        runs, native = [], Engine._joint_native

        def counted(self, fn, a, shard, *rest):      # the sharded stage runs, by entry point
            if shard is not None:
                runs.append(fn)
            return native(self, fn, a, shard, *rest)
        Engine._joint_native = counted
        n0 = N.collectives_issued(eng.lib)
        skipped = _suggest_all(joint_shard=(0, 1))   # a world of one rank: no exchange
        none = N.collectives_issued(eng.lib) - n0
        D.EXCHANGE_ALWAYS = True
        del runs[:]
        n0 = N.collectives_issued(eng.lib)
        got = _suggest_all(joint_shard=(0, 1))
        issued = N.collectives_issued(eng.lib) - n0
        ex = D.exchange_for(eng)
        q.put((ref, skipped, got, ex.comm is not None, none, issued, list(runs), None))
        ex.close()
    except Exception:
        import traceback
        q.put((None, None, None, None, None, None, None, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_one_nccl_rank_sends_its_records_through_rccl():
    """joint_shard=(0, 1) with dist.EXCHANGE_ALWAYS: the records of every joint
    stage run (flat: the root stage; tree: the branch stage; wide: the root
    stage) go through the RCCL all-gather, and the documents are the unsharded
    ones; without the switch a world of one rank exchanges nothing."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_worker, args=(_free_port(), q))
    p.start()
    ref, skipped, got, rccl, none, issued, runs, err = q.get(timeout=240)
    p.join(timeout=60)
    assert err is None, err
    assert rccl, 'the exchange did not take the RCCL path'
    assert skipped == ref and got == ref
    # one stage run per case (flat: quantised root group; tree: the mixed segmented stage; wide)
    assert sorted(runs) == ['tpe_joint_mseg_run', 'tpe_joint_quant_run', 'tpe_joint_wide_run'], runs
    assert none == 0 and issued >= len(runs), (none, issued, runs)
