"""bench.py's command line: a plain run is the default, the other legs and
the output dump are asked for."""
import bench


def test_plain_run_is_the_default():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_outputs_options():
    a = bench.parse(["--full", "--dump-outputs", "some/dir", "--no-pmc"])
    assert a.full is True and a.dump_outputs == "some/dir" and a.no_pmc is True
