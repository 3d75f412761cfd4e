"""GPU: do two trees write the same checkpoint files?  `run` trains learn(3) from a fixed seed with logging and exact_resume on (256 envs)
under the tree this file lies in and leaves model_*.pt / envstate_*.pt in OUT (HGYM_ASYNC_SAVE as set: once with 1, once with 0);
`compare` loads every such file of two OUT directories and compares key lists in order, tensors with torch.equal, scalars with ==.
    python tools/checkpoint_identity.py run OUT
    python tools/checkpoint_identity.py compare OUT_A OUT_B"""
import copy, glob, os, shutil, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "humanoid-gym_amd"))
import torch


def run(out):
    from humanoid.envs import task_registry
    from humanoid.utils import get_args
    a = get_args(["--task=humanoid_ppo", "--headless", "--num_envs", "256", "--seed", "5"])
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(name=a.task))
    train_cfg.runner.exact_resume = True
    env, _ = task_registry.make_env(name=a.task, args=a, env_cfg=env_cfg)
    runner, _ = task_registry.make_alg_runner(env=env, args=a, train_cfg=train_cfg, log_root=os.path.join(out, "logs"))
    runner.learn(num_learning_iterations=3, init_at_random_ep_len=True)
    runner.wait_for_saves()
    files = sorted(f for f in os.listdir(runner.log_dir) if f.endswith(".pt"))
    for f in files:
        shutil.copy(os.path.join(runner.log_dir, f), os.path.join(out, f))
    print("run %s HGYM_ASYNC_SAVE=%s: %s" % (out, os.environ.get("HGYM_ASYNC_SAVE", "1"), " ".join(files)))


def same(a, b, where, bad):
    if isinstance(a, dict) and isinstance(b, dict):
        if list(a) != list(b):
            bad.append("%s: keys %s != %s" % (where, list(a), list(b)))
        for k in a:
            if k in b:
                same(a[k], b[k], "%s[%r]" % (where, k), bad)
    elif torch.is_tensor(a) and torch.is_tensor(b):
        if a.dtype != b.dtype or a.shape != b.shape or not torch.equal(a, b):
            bad.append("%s: tensors differ" % where)
    elif isinstance(a, (list, tuple)) and type(a) is type(b) and len(a) == len(b):
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (where, i), bad)
    elif type(a) is not type(b) or a != b:
        bad.append("%s: %r != %r" % (where, a, b))


def compare(da, db):
    names = [sorted(os.path.basename(f) for pat in ("model_*.pt", "envstate_*.pt") for f in glob.glob(os.path.join(d, pat))) for d in (da, db)]
    bad = [] if names[0] == names[1] and names[0] else ["file lists: %s != %s" % tuple(names)]
    tensors = 0
    for f in names[0] if not bad else []:
        a, b = (torch.load(os.path.join(d, f), map_location="cpu") for d in (da, db))
        same(a, b, f, bad)
        count = lambda x: 1 if torch.is_tensor(x) else sum(count(v) for v in (x.values() if isinstance(x, dict) else x)) if isinstance(x, (dict, list, tuple)) else 0
        tensors += count(a)
    print("compare %s %s: %d files (%s), %d tensors: %s" % (da, db, len(names[0]), " ".join(names[0]), tensors, "IDENTICAL" if not bad else "DIFFERENT"))
    for line in bad:
        print("  " + line)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        os.makedirs(sys.argv[2], exist_ok=True)
        run(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
