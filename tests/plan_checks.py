"""
What the kernel tests of the four native plans (hip.FFTPlan, CorrPlan, HoloPlan, SSBPlan) share: one plan called on two
streams, and plans that go away completely.
"""


def three_calls_on_two_streams(call):
    """call(i, stream) for i = 0, 1, 2 on the default stream (stream None), a second stream and the default stream
    again, then ONE synchronisation.  Before every call its stream waits for the other one -- the plan's workspace is
    one: the calls run in order -- and then BOTH streams get matrix products to do, the other one twice as many: work
    of the call that is left on the other stream runs after the kernels of the call's own stream that need it."""
    import torch
    default = torch.cuda.current_stream()
    second = torch.cuda.Stream()
    a = torch.ones((4096, 4096), device='cuda')
    scratch = {default: torch.empty_like(a), second: torch.empty_like(a)}
    torch.cuda.synchronize()

    def busy(stream, n):
        with torch.cuda.stream(stream):
            for _ in range(n):
                torch.mm(a, a, out=scratch[stream])

    for i, (mine, other) in enumerate(((default, second), (second, default), (default, second))):
        mine.wait_stream(other)
        busy(mine, 4)
        busy(other, 8)
        call(i, None if mine is default else mine)
    torch.cuda.synchronize()


def assert_plans_go_away(make, footprint, what):
    """64 plans made and closed in a row: the free device memory after cycle 64 is less than `footprint` bytes -- ONE
    live plan of that kind -- below what it was after cycle 8.  A handle or workspace left behind per cycle would show
    56 times."""
    import torch
    free = {}
    for cycle in range(1, 65):
        make().close()
        if cycle in (8, 64):
            torch.cuda.synchronize()
            free[cycle] = torch.cuda.mem_get_info()[0]
    print(f"{what}: free memory after cycle 8 minus after cycle 64: {free[8] - free[64]} bytes (one plan: {footprint})")
    assert free[8] - free[64] < footprint, (what, free[8] - free[64], footprint)
