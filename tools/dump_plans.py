"""Dump every launch record the networks' schedules produce, one line per record, field for field:
    net prec tag kernel m_begin M ksplit pe side
for the refiner, the scorer and the scorer's features at every N in 1..FP_MAX_BATCH and the refiner on Register's shared crop at every
N in 2..42 * FP_MAX_INPLANE_STEPS, in f16 and bf16; FP8 and INT8 (after a one-frame calibration) at PLAN_SIZES; PLAN_SIZES under every
alternative schedule the test build keeps (conv_variant 3 / 5 / 7 / 8, smallm 0 / 2 / 3, enc_tail 0); and FP8 and INT8 at PLAN_SIZES under
every stage mask 0..15 of the 8-bit trunk (fpt_set_q8_blocks: a model per mask, on the calibration records of the first) and INT8 with the
8-bit residual stream (fpt_set_i8_stream).  Nothing is launched: the records come from fpt_plan_forward and the launch log.  Two builds decide alike exactly when their dumps are equal:

    FP_TEST_LIB_PATH=<build A>/libfoundationpose_amd_test.so python tools/dump_plans.py a.txt
    FP_TEST_LIB_PATH=<build B>/libfoundationpose_amd_test.so python tools/dump_plans.py b.txt && cmp a.txt b.txt

The last line printed is the dump's line count and SHA-256."""
import ctypes as C
import hashlib
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from foundationpose_cpp_amd import _lib  # noqa: E402

_lib.use_test_lib()
from foundationpose_cpp_amd import FoundationPose, synthetic as syn, weights as W  # noqa: E402
from foundationpose_cpp_amd.api import FP_PREC_BF16, FP_PREC_F16, FP_PREC_FP8, FP_PREC_INT8  # noqa: E402

N_MAX, STEPS_MAX = 2377, 56      # include/foundationpose_amd.h FP_MAX_BATCH, FP_MAX_INPLANE_STEPS
PLAN_SIZES = [1, 2, 5, 9, 14, 15, 28, 29, 32, 33, 64, 127, 252, 253, 1009, 2377]
REFINER, SCORER, SCORER_FEATURES = 0, 1, 2
KINDS = ("refiner", "scorer", "scorer-features")


def main(out_path):
    T = _lib.test_lib()
    T.fpt_plan_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    T.fpt_launch_log_get_all.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_int]
    mesh = syn.make_mesh()
    scene = syn.make_scene(mesh)
    weights_dir = tempfile.TemporaryDirectory()          # (kept to the end: a change of precision loads the weights again)
    rp, sp = os.path.join(weights_dir.name, "r.fpw"), os.path.join(weights_dir.name, "s.fpw")
    W.pack_synthetic("refiner", rp)
    W.pack_synthetic("scorer", sp)
    model = FoundationPose(mesh, scene.K, rp, sp)
    models = [model]                                      # plan() asks the last one
    sha, lines = hashlib.sha256(), 0
    out = open(out_path, "w")

    def emit(text):
        nonlocal lines
        out.write(text + "\n")
        sha.update((text + "\n").encode())
        lines += 1

    def plan(what, kind, N, shared=0):
        emit(f"# {what} {KINDS[kind]} N={N} shared={shared}")
        T.fpt_launch_log_arm(1)
        rc = T.fpt_plan_forward(models[-1]._h, kind, N, shared)
        T.fpt_launch_log_arm(0)
        if rc != 0:
            emit("plan-only failed: " + T.fp_last_error().decode())
        n = T.fpt_launch_log_count()
        f = (C.c_int * (7 * max(n, 1)))()
        names = C.create_string_buffer(96 * max(n, 1))
        assert T.fpt_launch_log_get_all(f, names, 96, n) == n
        for i in range(n):
            net, prec, side, m_begin, M, ksplit, pe = f[7 * i:7 * i + 7]
            tag, _, kern = names.raw[96 * i:96 * (i + 1)].split(b"\0", 1)[0].decode().rpartition("/")
            emit(f"{net} {prec} {tag} {kern} {m_begin} {M} {ksplit} {pe} {side}")
        T.fpt_launch_log_clear()

    def sweep(what, sizes, shared_max):
        for N in sizes:
            for kind in (REFINER, SCORER, SCORER_FEATURES):
                plan(what, kind, N)
            if 1 < N <= shared_max:
                plan(what, REFINER, N, 1)

    try:
        for name, prec in (("f16", FP_PREC_F16), ("bf16", FP_PREC_BF16)):
            model.set_precision(prec)
            sweep(name, range(N_MAX, 0, -1), 42 * STEPS_MAX)      # (largest first: the buffers grow once)
        model.set_precision(FP_PREC_F16)
        for setter, values in (("fpt_set_conv_variant", (3, 5, 7, 8, 0)), ("fpt_set_smallm", (0, 2, 3, 1)), ("fpt_set_enc_tail", (0, 1))):
            for v in values[:-1]:
                getattr(T, setter)(v)
                for name, prec in (("f16", FP_PREC_F16), ("bf16", FP_PREC_BF16)):
                    model.set_precision(prec)
                    sweep(f"{setter[8:]}={v} {name}", PLAN_SIZES, 42 * STEPS_MAX)
            getattr(T, setter)(values[-1])                        # back to the default
        model.set_precision(FP_PREC_F16)
        blobs = []
        for name, prec in (("fp8", FP_PREC_FP8), ("int8", FP_PREC_INT8)):
            model.calibrate(scene.rgb, scene.depth, scene.mask, mesh.name, prec)
            blobs.append(model.get_calibration_blob(prec))
            model.set_precision(prec)
            sweep(name, PLAN_SIZES, 42 * STEPS_MAX)
            model.set_precision(FP_PREC_F16)
        for mask in range(16):                                # a network keeps the mask it was loaded with: a model per mask
            T.fpt_set_q8_blocks(mask)
            models.append(FoundationPose(mesh, scene.K, rp, sp))
            try:
                for blob in blobs:
                    models[-1].set_calibration_blob(blob)
                for name, prec in (("fp8", FP_PREC_FP8), ("int8", FP_PREC_INT8)):
                    models[-1].set_precision(prec)
                    sweep(f"q8_blocks={mask} {name}", PLAN_SIZES, 42 * STEPS_MAX)
                    if mask == 15 and prec == FP_PREC_INT8:
                        T.fpt_set_i8_stream(1)
                        sweep(f"i8_stream=1 {name}", PLAN_SIZES, 42 * STEPS_MAX)
                        T.fpt_set_i8_stream(0)
            finally:
                models.pop().close()
        T.fpt_set_q8_blocks(15)
    finally:
        T.fpt_set_i8_stream(0)
        T.fpt_set_q8_blocks(15)
        model.close()
        out.close()
        weights_dir.cleanup()
    print(f"{out_path}: {lines} lines, sha256 {sha.hexdigest()}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "plans.txt")
