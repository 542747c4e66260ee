"""What the tests of the `hammlet` driver share: where the binary is, and one run of it on a trace."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "hammlet_amd", "hammlet")


def run_cli(tmp, x, flags, outputs, one_gpu=False, prefix="g-", overwrite=True, timeout=None):
    """`hammlet -raw <x> -o <tmp>/<prefix> .csv -a [-w] <flags> -O <outputs>`: the finished process, its output captured.
    one_gpu: the process sees the first GPU only, so that the chains of -chains N share it; timeout: seconds, the run's own."""
    raw = os.path.join(tmp, "in.f32")
    x.tofile(raw)
    env = dict(os.environ)
    if one_gpu:
        env["HIP_VISIBLE_DEVICES"] = "0"
    return subprocess.run([CLI, "-raw", raw, "-o", os.path.join(tmp, prefix), ".csv", "-a"] + (["-w"] if overwrite else []) + flags.split() + ["-O"] + outputs,
                          capture_output=True, text=True, env=env, timeout=timeout)
