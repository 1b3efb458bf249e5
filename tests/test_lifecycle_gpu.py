"""GPU: a context and its planner give back all the device memory they took.

One cycle on the small parity grid: create the context and the planner, run one short flight, one update and one replan
(so that the set-ups that allocate on first use have run: the update flow, the stamp's scratch, the crop lists, the mark
logs, the flight), destroy the planner, then the context.  Free device memory is read after a device synchronise at the
end of every cycle; torch's caching allocator and the runtime's own pools have settled after two cycles, so cycle 2 is the
baseline.

The bound is not a measurement.  Before the resources had one owner, sogm_planner_destroy did not free the flight's
workgroup-start log: 8 x FL_WG_LOG words of 8 bytes (FL_WG_LOG from csrc/sogm_planner.hpp) per planner that ever flew.
Free memory after the last of N cycles may be lower than after cycle 2 by at most HALF of what that leak amounts to over
the same N - 2 cycles; N = 32 makes the bound 3.75 MiB, several times the 2 MiB granularity at which the device's free
memory moves.  The code before the change fails: measured there, 2 MiB less every fourth cycle, a drift of 16 MiB."""
import gc
import importlib
import os
import re

import pytest

pytestmark = pytest.mark.gpu

N_CYCLES = 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fl_wg_log():
    text = open(os.path.join(ROOT, "pred-occ-planner_amd", "csrc", "sogm_planner.hpp")).read()
    return int(re.search(r"^#define\s+FL_WG_LOG\s+(\d+)\s*$", text, re.M).group(1))


def _cycle(driver):
    import torch
    sw = driver.SwarmTick("parity", 4, moving_world=True, prestamp=False)
    sw.fly(3)  # (a SwarmTick flies from tick 0 only: the flight first)
    sw.step()  # one update + one replan
    torch.cuda.synchronize()
    assert sw.planner.flow_failures() == (0, 0)
    sw.close()  # the planner, then the context
    del sw
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_create_use_destroy_cycles_give_their_device_memory_back(pop):
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    leak_per_planner = 8 * _fl_wg_log() * 8
    allowed = (N_CYCLES - 2) * leak_per_planner // 2
    free = [_cycle(driver) for _ in range(N_CYCLES)]
    drift = free[1] - free[-1]
    print(f"free device memory after cycle 2: {free[1]}, after cycle {N_CYCLES}: {free[-1]}, drift {drift} B "
          f"({drift / 1024:.0f} KiB), allowed {allowed} B; per cycle (MiB): {[round(f / 2**20, 2) for f in free]}")
    assert drift <= allowed, (drift, allowed)
