"""ctypes binding to libethrex_mi355.so (the gfx950 HIP core).

Loads the in-tree shared library built by __graft_entry__.build().  Import
fails loudly if the library is absent: the product path never falls back
to CPU.
"""
import array
import ctypes
import os

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libethrex_mi355.so")

if not os.path.exists(_SO):
    raise ImportError(
        f"HIP core library missing: {_SO}. Run __graft_entry__.build() "
        "(hipcc --offload-arch=gfx950). The product path has no CPU fallback.")

_lib = ctypes.CDLL(_SO)

EM_OK = 0
EM_ERR_POINT = 1
EM_ERR_INPUT = 2
EM_ERR_HIP = 3

_lib.ethrex_mi355_version.restype = ctypes.c_char_p
_lib.ethrex_mi355_last_error.restype = ctypes.c_char_p
for _f in ("device_count", "set_device", "bn254_g1_add", "bn254_g1_mul",
           "bn254_g1_msm", "bn254_fr_ntt", "bn254_g1_combine",
           "msm_plan_create", "msm_plan_destroy", "msm_upload_points",
           "msm_gen_points", "msm_download_points", "msm_upload_scalars",
           "msm_run", "msm_run_partial", "msm_run_async", "msm_sync",
           "msm_run_partial_async", "msm_wait_one", "bn254_g1_combine_cpu",
           "msm_last_times", "msm_combine", "msm_scalars_from_ntt",
           "msm_fb_info", "msm_download_fb_rows", "ntt_device_data",
           "ntt_plan_create", "ntt_plan_destroy", "ntt_upload", "ntt_run",
           "ntt_download", "ntt_last_times", "ntt_fill_from_digests",
           "ntt_last_fill_ms", "keccak_device_digests",
           "ntt_run_coset", "bn254_fr_coset_ntt", "quot_plan_create",
           "quot_plan_destroy", "quot_upload", "quot_load_device",
           "quot_mul_ab_into_c", "quot_run", "quot_download",
           "quot_device_data", "quot_last_times", "r1cs_plan_create",
           "r1cs_plan_destroy", "r1cs_upload_matrix", "r1cs_upload_witness",
           "r1cs_witness_from_device", "r1cs_eval", "r1cs_download",
           "r1cs_device_data", "r1cs_last_times"):
    getattr(_lib, f"ethrex_mi355_{_f}").restype = ctypes.c_int


class HipCoreError(RuntimeError):
    def __init__(self, rc, what):
        self.rc = rc
        super().__init__(f"{what}: rc={rc} ({last_error()})")


def _check(rc, what):
    if rc != EM_OK:
        raise HipCoreError(rc, what)


def _buf(b):
    return (ctypes.c_uint8 * len(b)).from_buffer_copy(b)


def version() -> str:
    return _lib.ethrex_mi355_version().decode()


def last_error() -> str:
    return (_lib.ethrex_mi355_last_error() or b"").decode()


def device_count() -> int:
    n = ctypes.c_int(0)
    _lib.ethrex_mi355_device_count(ctypes.byref(n))
    return n.value


def set_device(d: int):
    _check(_lib.ethrex_mi355_set_device(ctypes.c_int(d)), "set_device")


def g1_add(p1: bytes, p2: bytes):
    out = (ctypes.c_uint8 * 64)()
    rc = _lib.ethrex_mi355_bn254_g1_add(_buf(p1), _buf(p2), out)
    return rc, bytes(out)


def g1_mul(point: bytes, scalar: bytes):
    out = (ctypes.c_uint8 * 64)()
    rc = _lib.ethrex_mi355_bn254_g1_mul(_buf(point), _buf(scalar), out)
    return rc, bytes(out)


def g1_msm(points: bytes, scalars: bytes, n: int):
    out = (ctypes.c_uint8 * 64)()
    rc = _lib.ethrex_mi355_bn254_g1_msm(_buf(points), _buf(scalars),
                                        ctypes.c_size_t(n), out)
    return rc, bytes(out)


def fr_ntt(elems: bytes, n: int, inverse: bool):
    buf = _buf(elems)
    rc = _lib.ethrex_mi355_bn254_fr_ntt(buf, ctypes.c_size_t(n),
                                        ctypes.c_int(1 if inverse else 0))
    return rc, bytes(buf)


def coset_ntt(elems: bytes, n: int, inverse: bool):
    """One-shot coset transform (generator g = 5): forward is the NTT of
    a_i g^i, inverse the iNTT followed by g^-i."""
    buf = _buf(elems)
    rc = _lib.ethrex_mi355_bn254_fr_coset_ntt(
        buf, ctypes.c_size_t(n), ctypes.c_int(1 if inverse else 0))
    return rc, bytes(buf)


def g1_combine(jacobians: bytes, count: int):
    out = (ctypes.c_uint8 * 64)()
    rc = _lib.ethrex_mi355_bn254_g1_combine(_buf(jacobians),
                                            ctypes.c_size_t(count), out)
    return rc, bytes(out)


def g1_combine_cpu(jacobians: bytes, count: int) -> bytes:
    """Host-side combine of the N>1 exchange payload (world-size 96-B
    Jacobian partials) — boundary glue; keeps GPU streams untouched while
    pipelined steps are in flight."""
    out = (ctypes.c_uint8 * 64)()
    rc = _lib.ethrex_mi355_bn254_g1_combine_cpu(_buf(jacobians),
                                                ctypes.c_size_t(count), out)
    if rc != EM_OK:
        raise HipCoreError(rc, "bn254_g1_combine_cpu")
    return bytes(out)


def gen_fr(seed: int, n: int) -> bytes:
    """Deterministic Fr elements (host-side; BASELINE.md input scheme)."""
    out = (ctypes.c_uint8 * (32 * n))()
    _lib.ethrex_mi355_gen_fr(ctypes.c_uint64(seed), ctypes.c_size_t(n), out)
    return bytes(out)


class _MsmPlanBase:
    """What the four device-resident MSM plans share.  A subclass names its
    ABI family (functions ethrex_mi355_<_PREFIX>_<op>, error labels
    <_PREFIX>_<op>), its affine and Jacobian point sizes, and in _OPS every
    op it may call."""

    _PREFIX = None
    _AFF = 0   # bytes of an affine point (points, run, run_async)
    _JAC = 0   # bytes of a Jacobian partial (run_partial)
    _OPS = ("plan_create", "plan_destroy", "upload_points", "gen_points",
            "download_points", "upload_scalars", "run", "run_partial",
            "run_async", "sync", "last_times")

    @classmethod
    def _fn(cls, op):
        if op not in cls._OPS:
            raise AttributeError(f"{cls.__name__}: undeclared op {op}")
        return getattr(_lib, f"ethrex_mi355_{cls._PREFIX}_{op}")

    def _call(self, op, *args):
        _check(self._fn(op)(self._p, *args), f"{self._PREFIX}_{op}")

    def _call_out(self, op, nbytes):
        out = (ctypes.c_uint8 * nbytes)()
        self._call(op, out)
        return out

    def __init__(self, n: int):
        self.n = n
        self._p = ctypes.c_void_p()
        self._pending = []
        _check(self._fn("plan_create")(ctypes.c_size_t(n),
                                       ctypes.byref(self._p)),
               f"{self._PREFIX}_plan_create")

    def upload_points(self, points: bytes):
        self._call("upload_points", _buf(points))

    def gen_points(self, start: int = 0):
        self._call("gen_points", ctypes.c_uint64(start))

    def download_points(self) -> bytes:
        return bytes(self._call_out("download_points", self._AFF * self.n))

    def upload_scalars(self, scalars: bytes):
        self._call("upload_scalars", _buf(scalars))

    def _scalars_from_ntt(self, src, offset):
        # any source with a device_data() -> (ptr, n) accessor: an NttPlan
        # or a QuotPlan (whose h feeds the Z-basis MSM)
        ptr, nn = src.device_data()
        if offset + self.n > nn:
            raise HipCoreError(EM_ERR_INPUT,
                               f"scalars_from_ntt: offset {offset} + n "
                               f"{self.n} exceeds NTT size {nn}")
        self._call("scalars_from_ntt", ptr, ctypes.c_uint64(offset))

    def run(self) -> bytes:
        return bytes(self._call_out("run", self._AFF))

    def run_partial(self) -> bytes:
        return bytes(self._call_out("run_partial", self._JAC))

    def run_async(self):
        """Enqueue one pipelined MSM step (sort chain of the next step
        overlaps this step's compute chain).  Result delivered at sync()."""
        self._pending.append(self._call_out("run_async", self._AFF))

    def sync(self) -> bytes:
        """Drain the pipeline; returns the LAST pipelined result."""
        self._call("sync")
        outs = [bytes(b) for b in self._pending]
        self._pending = []
        return outs[-1] if outs else b""

    def last_times(self):
        t = (ctypes.c_double * 5)()
        self._call("last_times", t)
        return {"digits_sort_ms": t[0], "bucket_acc_ms": t[1],
                "reduce_ms": t[2], "combine_ms": t[3], "total_ms": t[4]}

    def destroy(self):
        if self._p:
            self._fn("plan_destroy")(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class MsmPlan(_MsmPlanBase):
    """Device-resident MSM plan: upload once, run many (bench/pipeline)."""

    _PREFIX, _AFF, _JAC = "msm", 64, 96
    _OPS = _MsmPlanBase._OPS + (
        "fb_info", "download_fb_rows", "run_partial_async", "wait_one",
        "scalars_from_ntt", "combine")

    def last_times(self):
        t = super().last_times()
        t["fb_precompute_ms"] = self._fb_info()[1]
        return t

    def _fb_info(self):
        c = ctypes.c_int(0)
        ms = ctypes.c_double(0.0)
        nbytes = ctypes.c_uint64(0)
        self._call("fb_info", ctypes.byref(c), ctypes.byref(ms),
                   ctypes.byref(nbytes))
        return c.value, ms.value, nbytes.value

    @property
    def fixed_base(self) -> int:
        """Window bits c of the merged fixed-base mode this plan runs
        (table of 2^(c*w) * P_i built when the points are loaded), or 0
        when it runs the separate-window path."""
        return self._fb_info()[0]

    @property
    def fb_table_bytes(self) -> int:
        return self._fb_info()[2]

    def download_fb_rows(self, w: int, start: int, count: int) -> bytes:
        """Rows [start, start+count) of window w of the fixed-base table
        as 64-byte affine points (parity tests)."""
        out = (ctypes.c_uint8 * (64 * count))()
        self._call("download_fb_rows", ctypes.c_int(w),
                   ctypes.c_size_t(start), ctypes.c_size_t(count), out)
        return bytes(out)

    def run_partial_async(self):
        """Pipelined shard step: delivers the 96-B Jacobian partial at
        sync() (the N>1 exchange payload)."""
        self._pending.append(self._call_out("run_partial_async", self._JAC))

    def wait_one(self) -> bytes:
        """Deliver ONLY the oldest pending pipelined step (later steps keep
        running on the GPU).  The N>1 loop exchanges step k's partial while
        the GPU computes step k+1."""
        if not self._pending:
            return b""
        self._call("wait_one")
        return bytes(self._pending.pop(0))

    def scalars_from_ntt(self, ntt_plan, offset: int = 0):
        """wrap-pipeline handoff: take this plan's n scalars from the NTT
        plan's device-resident output at element `offset` (on-device, no
        PCIe; the sp1.rs:122-134 wrap flow feeds the witness NTT output
        into the proving MSM)."""
        self._scalars_from_ntt(ntt_plan, offset)

    def combine(self, jacobians: bytes, count: int) -> bytes:
        """combine Jacobian partials reusing this plan's device buffers"""
        out = (ctypes.c_uint8 * 64)()
        self._call("combine", _buf(jacobians), ctypes.c_size_t(count), out)
        return bytes(out)


class NttPlan:
    def __init__(self, n: int):
        self.n = n
        self._p = ctypes.c_void_p()
        _check(_lib.ethrex_mi355_ntt_plan_create(ctypes.c_size_t(n),
                                                 ctypes.byref(self._p)),
               "ntt_plan_create")

    def upload(self, elems: bytes):
        _check(_lib.ethrex_mi355_ntt_upload(self._p, _buf(elems)), "ntt_upload")

    def run(self, inverse: bool = False):
        _check(_lib.ethrex_mi355_ntt_run(self._p,
                                         ctypes.c_int(1 if inverse else 0)),
               "ntt_run")

    def run_coset(self, inverse: bool = False):
        """coset transform (g = 5): forward = NTT of a_i g^i, inverse =
        iNTT then g^-i; same buffer rules as run()."""
        _check(_lib.ethrex_mi355_ntt_run_coset(
            self._p, ctypes.c_int(1 if inverse else 0)), "ntt_run_coset")

    def download(self) -> bytes:
        out = (ctypes.c_uint8 * (32 * self.n))()
        _check(_lib.ethrex_mi355_ntt_download(self._p, out), "ntt_download")
        return bytes(out)

    def device_data(self):
        """(device pointer, n) of the current resident vector (fe4m)"""
        ptr = ctypes.c_void_p()
        nn = ctypes.c_size_t(0)
        _check(_lib.ethrex_mi355_ntt_device_data(
            self._p, ctypes.byref(ptr), ctypes.byref(nn)), "ntt_device_data")
        return ptr, nn.value

    def last_times(self):
        t = (ctypes.c_double * 3)()
        _check(_lib.ethrex_mi355_ntt_last_times(self._p, t), "ntt_last_times")
        return {"bitrev_ms": t[0], "stages_ms": t[1], "total_ms": t[2]}

    def fill_from_digests(self, keccak_plan, domain: bytes):
        """witness binding: fill the n resident elements with wrap vector
        v1 (witness.wrap_vector) expanded ON DEVICE from the keccak plan's
        resident digests — replaces upload(); nothing crosses PCIe."""
        if len(domain) != 32:
            raise HipCoreError(EM_ERR_INPUT,
                               "fill_from_digests: domain must be 32 bytes")
        ptr, m = keccak_plan.device_digests()
        _check(_lib.ethrex_mi355_ntt_fill_from_digests(
            self._p, ptr, ctypes.c_size_t(m), _buf(domain)),
            "ntt_fill_from_digests")

    def last_fill_ms(self) -> float:
        ms = ctypes.c_double(0)
        _check(_lib.ethrex_mi355_ntt_last_fill_ms(self._p, ctypes.byref(ms)),
               "ntt_last_fill_ms")
        return ms.value

    def destroy(self):
        if self._p:
            _lib.ethrex_mi355_ntt_plan_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class QuotPlan:
    """Device-resident Groth16 quotient polynomial: three evaluation
    vectors a, b, c (slots 0, 1, 2) -> h = coset_inv((a~ b~ - c~) /
    (g^n - 1)), x~ = coset_fwd(intt(x)).  One twiddle set, three vectors
    and one work buffer; run() consumes the slots."""

    def __init__(self, n: int):
        self.n = n
        self._p = ctypes.c_void_p()
        _check(_lib.ethrex_mi355_quot_plan_create(ctypes.c_size_t(n),
                                                  ctypes.byref(self._p)),
               "quot_plan_create")

    def upload(self, which: int, elems: bytes):
        if len(elems) != 32 * self.n:
            raise HipCoreError(EM_ERR_INPUT,
                               f"quot_upload: need {32 * self.n} bytes")
        _check(_lib.ethrex_mi355_quot_upload(self._p, ctypes.c_int(which),
                                             _buf(elems)), "quot_upload")

    def load_from_ntt(self, which: int, nplan):
        """copy the NTT plan's current resident vector into a slot
        (device to device; after fill_from_digests or a run)"""
        ptr, nn = nplan.device_data()
        if nn != self.n:
            raise HipCoreError(EM_ERR_INPUT,
                               f"quot_load_from_ntt: size {nn} != {self.n}")
        _check(_lib.ethrex_mi355_quot_load_device(
            self._p, ctypes.c_int(which), ptr), "quot_load_device")

    def load_from_r1cs(self, which: int, rplan, matrix: int):
        """copy an R1csPlan result (matrix 0 = A z, 1 = B z, 2 = C z) into a
        slot, device to device"""
        ptr, nn = rplan.device_data(matrix)
        if nn != self.n:
            raise HipCoreError(EM_ERR_INPUT,
                               f"quot_load_from_r1cs: size {nn} != {self.n}")
        _check(_lib.ethrex_mi355_quot_load_device(
            self._p, ctypes.c_int(which), ptr), "quot_load_device")

    def mul_ab_into_c(self):
        _check(_lib.ethrex_mi355_quot_mul_ab_into_c(self._p),
               "quot_mul_ab_into_c")

    def run(self):
        _check(_lib.ethrex_mi355_quot_run(self._p), "quot_run")

    def download(self) -> bytes:
        out = (ctypes.c_uint8 * (32 * self.n))()
        _check(_lib.ethrex_mi355_quot_download(self._p, out),
               "quot_download")
        return bytes(out)

    def device_data(self):
        """(device pointer, n) of h (fe4m); valid until the next
        load/run/destroy — the MsmPlan.scalars_from_ntt source"""
        ptr = ctypes.c_void_p()
        nn = ctypes.c_size_t(0)
        _check(_lib.ethrex_mi355_quot_device_data(
            self._p, ctypes.byref(ptr), ctypes.byref(nn)),
            "quot_device_data")
        return ptr, nn.value

    def last_times(self):
        t = (ctypes.c_double * 5)()
        _check(_lib.ethrex_mi355_quot_last_times(self._p, t),
               "quot_last_times")
        return {"intt3_ms": t[0], "coset_ntt3_ms": t[1],
                "pointwise_ms": t[2], "coset_intt_ms": t[3],
                "total_ms": t[4]}

    def destroy(self):
        if self._p:
            _lib.ethrex_mi355_quot_plan_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class R1csPlan:
    """Device-resident R1CS evaluation: the three sparse constraint
    matrices A, B, C (which = 0, 1, 2; CSR, uploaded once and repacked on
    the host) times the witness vector z of n_vars elements.  The results
    are n resident elements each (rows past the matrix are zero) and feed
    QuotPlan.load_from_r1cs without leaving the device."""

    def __init__(self, n: int, n_vars: int):
        self.n = n
        self.n_vars = n_vars
        self._p = ctypes.c_void_p()
        _check(_lib.ethrex_mi355_r1cs_plan_create(
            ctypes.c_size_t(n), ctypes.c_size_t(n_vars),
            ctypes.byref(self._p)), "r1cs_plan_create")

    def upload_matrix(self, which: int, row_offs, cols, coeffs_bytes: bytes):
        """row_offs: n_rows + 1 offsets; cols: nnz column indices;
        coeffs_bytes: nnz 32-byte big-endian canonical coefficients"""
        try:
            row_offs = array.array("Q", row_offs)
            cols = array.array("I", cols)
        except (OverflowError, TypeError):
            raise HipCoreError(EM_ERR_INPUT,
                               "r1cs_upload_matrix: offsets are u64, "
                               "columns u32") from None
        if not row_offs:
            raise HipCoreError(EM_ERR_INPUT,
                               "r1cs_upload_matrix: row_offs is empty")
        if len(coeffs_bytes) != 32 * len(cols):
            raise HipCoreError(EM_ERR_INPUT,
                               f"r1cs_upload_matrix: need {32 * len(cols)} "
                               "coefficient bytes")
        if row_offs[-1] != len(cols):
            raise HipCoreError(EM_ERR_INPUT,
                               f"r1cs_upload_matrix: {len(cols)} columns for "
                               f"{row_offs[-1]} entries")
        n_rows = len(row_offs) - 1
        offs = (ctypes.c_uint64 * len(row_offs)).from_buffer(row_offs)
        # one spare element keeps the pointers of an empty matrix non-null
        cols.append(0)
        carr = (ctypes.c_uint32 * len(cols)).from_buffer(cols)
        _check(_lib.ethrex_mi355_r1cs_upload_matrix(
            self._p, ctypes.c_int(which), offs, carr,
            _buf(coeffs_bytes + b"\x00"),
            ctypes.c_size_t(n_rows)), "r1cs_upload_matrix")

    def upload_witness(self, z_bytes: bytes):
        if len(z_bytes) != 32 * self.n_vars:
            raise HipCoreError(EM_ERR_INPUT,
                               f"r1cs_upload_witness: need "
                               f"{32 * self.n_vars} bytes")
        _check(_lib.ethrex_mi355_r1cs_upload_witness(self._p, _buf(z_bytes)),
               "r1cs_upload_witness")

    def witness_from(self, src, offset: int = 0):
        """take z from n_vars resident elements of any plan with a
        device_data() -> (ptr, n) accessor, at element `offset`"""
        ptr, nn = src.device_data()
        if offset < 0 or offset + self.n_vars > nn:
            raise HipCoreError(EM_ERR_INPUT,
                               f"r1cs_witness_from: offset {offset} + n_vars "
                               f"{self.n_vars} exceeds source size {nn}")
        _check(_lib.ethrex_mi355_r1cs_witness_from_device(
            self._p, ptr, ctypes.c_uint64(offset)),
            "r1cs_witness_from_device")

    def eval(self, which: int):
        _check(_lib.ethrex_mi355_r1cs_eval(self._p, ctypes.c_int(which)),
               "r1cs_eval")

    def eval_all(self):
        for which in range(3):
            self.eval(which)

    def download(self, which: int) -> bytes:
        out = (ctypes.c_uint8 * (32 * self.n))()
        _check(_lib.ethrex_mi355_r1cs_download(self._p, ctypes.c_int(which),
                                               out), "r1cs_download")
        return bytes(out)

    def device_data(self, which: int):
        """(device pointer, n) of M_which z (fe4m); valid until the next
        eval / upload_matrix of that matrix or destroy"""
        ptr = ctypes.c_void_p()
        nn = ctypes.c_size_t(0)
        _check(_lib.ethrex_mi355_r1cs_device_data(
            self._p, ctypes.c_int(which), ctypes.byref(ptr),
            ctypes.byref(nn)), "r1cs_device_data")
        return ptr, nn.value

    def last_times(self):
        t = (ctypes.c_double * 3)()
        _check(_lib.ethrex_mi355_r1cs_last_times(self._p, t),
               "r1cs_last_times")
        return {"a_ms": t[0], "b_ms": t[1], "c_ms": t[2]}

    def destroy(self):
        if self._p:
            _lib.ethrex_mi355_r1cs_plan_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ==== BLS12-381 G1 (bls_blst.rs semantics) ====

for _f in ("bls12381_g1_add", "bls12381_g1_mul", "bls12381_g1_msm",
           "bls12381_g1_combine", "bls_msm_plan_create", "bls_msm_plan_destroy",
           "bls_msm_upload_points", "bls_msm_gen_points",
           "bls_msm_download_points", "bls_msm_upload_scalars", "bls_msm_run",
           "bls_msm_run_async", "bls_msm_sync", "bls12381_g2_add",
           "bls12381_g2_mul", "bls12381_g2_msm", "bls_g2_msm_plan_create",
           "bls_g2_msm_plan_destroy", "bls_g2_msm_upload_points",
           "bls_g2_msm_gen_points", "bls_g2_msm_download_points",
           "bls_g2_msm_upload_scalars", "bls_g2_msm_run",
           "bls_g2_msm_run_async", "bls_g2_msm_sync",
           "bls_g2_msm_run_partial", "bls_g2_msm_last_times",
           "keccak256_batch", "keccak_plan_create", "keccak_plan_destroy",
           "keccak_upload", "keccak_run", "keccak_download",
           "keccak_last_ms", "mpt_create", "mpt_destroy", "mpt_max_depth",
           "mpt_level_encode", "mpt_level_set_hashes", "mpt_root",
           "bls_msm_run_partial", "bls_msm_last_times", "bls_msm_precompute"):
    getattr(_lib, f"ethrex_mi355_{_f}").restype = ctypes.c_int


def bls_g1_add(p1: bytes, p2: bytes):
    out = (ctypes.c_uint8 * 96)()
    rc = _lib.ethrex_mi355_bls12381_g1_add(_buf(p1), _buf(p2), out)
    return rc, bytes(out)


def bls_g1_mul(point: bytes, scalar: bytes):
    out = (ctypes.c_uint8 * 96)()
    rc = _lib.ethrex_mi355_bls12381_g1_mul(_buf(point), _buf(scalar), out)
    return rc, bytes(out)


def bls_g1_msm(points: bytes, scalars: bytes, n: int):
    out = (ctypes.c_uint8 * 96)()
    rc = _lib.ethrex_mi355_bls12381_g1_msm(_buf(points), _buf(scalars),
                                           ctypes.c_size_t(n), out)
    return rc, bytes(out)


def bls_g1_combine(jacobians: bytes, count: int):
    out = (ctypes.c_uint8 * 96)()
    rc = _lib.ethrex_mi355_bls12381_g1_combine(_buf(jacobians),
                                               ctypes.c_size_t(count), out)
    return rc, bytes(out)


def bls_gen_fr(seed: int, n: int) -> bytes:
    out = (ctypes.c_uint8 * (32 * n))()
    _lib.ethrex_mi355_bls_gen_fr(ctypes.c_uint64(seed), ctypes.c_size_t(n), out)
    return bytes(out)


class BlsMsmPlan(_MsmPlanBase):
    """Device-resident BLS12-381 G1 MSM plan (blob-KZG commitment shape)."""

    _PREFIX, _AFF, _JAC = "bls_msm", 96, 144
    _OPS = _MsmPlanBase._OPS + ("precompute",)

    def precompute(self):
        """fixed-base table (setup points fixed across blobs)"""
        self._call("precompute")


def bls_g2_add(p1: bytes, p2: bytes):
    out = (ctypes.c_uint8 * 192)()
    rc = _lib.ethrex_mi355_bls12381_g2_add(_buf(p1), _buf(p2), out)
    return rc, bytes(out)


def bls_g2_mul(point: bytes, scalar: bytes):
    out = (ctypes.c_uint8 * 192)()
    rc = _lib.ethrex_mi355_bls12381_g2_mul(_buf(point), _buf(scalar), out)
    return rc, bytes(out)


def bls_g2_msm(points: bytes, scalars: bytes, n: int):
    out = (ctypes.c_uint8 * 192)()
    rc = _lib.ethrex_mi355_bls12381_g2_msm(_buf(points), _buf(scalars),
                                           ctypes.c_size_t(n), out)
    return rc, bytes(out)


class BlsG2MsmPlan(_MsmPlanBase):
    """Device-resident BLS12-381 G2 MSM plan (EIP-2537 G2MSM shape)."""

    _PREFIX, _AFF, _JAC = "bls_g2_msm", 192, 288


# ==== BN254 G2 (the Groth16 B-query; EIP-197 byte semantics) ====
# 128-byte points x.c1||x.c0||y.c1||y.c0 (imaginary part first, canonical
# 32-B BE coords), all-zero = identity; scalars 32-B BE reduced mod r;
# mul/msm/upload_points enforce the r-subgroup check, add on-curve only.

for _f in ("bn254_g2_add", "bn254_g2_mul", "bn254_g2_msm",
           "bn254_g2_msm_plan_create", "bn254_g2_msm_plan_destroy",
           "bn254_g2_msm_upload_points", "bn254_g2_msm_gen_points",
           "bn254_g2_msm_download_points", "bn254_g2_msm_upload_scalars",
           "bn254_g2_msm_run", "bn254_g2_msm_run_partial",
           "bn254_g2_msm_run_async", "bn254_g2_msm_sync",
           "bn254_g2_msm_last_times", "bn254_g2_msm_scalars_from_ntt"):
    getattr(_lib, f"ethrex_mi355_{_f}").restype = ctypes.c_int


def bn254_g2_add(p1: bytes, p2: bytes):
    out = (ctypes.c_uint8 * 128)()
    rc = _lib.ethrex_mi355_bn254_g2_add(_buf(p1), _buf(p2), out)
    return rc, bytes(out)


def bn254_g2_mul(point: bytes, scalar: bytes):
    out = (ctypes.c_uint8 * 128)()
    rc = _lib.ethrex_mi355_bn254_g2_mul(_buf(point), _buf(scalar), out)
    return rc, bytes(out)


def bn254_g2_msm(points: bytes, scalars: bytes, n: int):
    out = (ctypes.c_uint8 * 128)()
    rc = _lib.ethrex_mi355_bn254_g2_msm(_buf(points), _buf(scalars),
                                        ctypes.c_size_t(n), out)
    return rc, bytes(out)


class Bn254G2MsmPlan(_MsmPlanBase):
    """Device-resident BN254 G2 MSM plan (Groth16 B2 = sum w_i * B_i)."""

    _PREFIX, _AFF, _JAC = "bn254_g2_msm", 128, 192
    _OPS = _MsmPlanBase._OPS + ("scalars_from_ntt",)

    def scalars_from_ntt(self, ntt_plan, offset: int = 0):
        """take this plan's n scalars from an NttPlan / QuotPlan's
        device-resident vector at element `offset` (on device, no PCIe):
        the witness vector feeds B2 directly"""
        self._scalars_from_ntt(ntt_plan, offset)


def keccak256_batch(msgs: bytes, offsets, n: int):
    """Batched Ethereum keccak256 (one-shot, PCIe-inclusive); offsets is a
    list of n+1 byte offsets into msgs."""
    offs = (ctypes.c_uint64 * (n + 1))(*offsets)
    out = (ctypes.c_uint8 * (32 * n))()
    rc = _lib.ethrex_mi355_keccak256_batch(
        _buf(msgs) if msgs else None, offs, ctypes.c_size_t(n), out)
    return rc, bytes(out)


class KeccakPlan:
    """Device-resident batched keccak256 (witness/trie hashing shape)."""

    def __init__(self, max_bytes: int, max_n: int):
        self._p = ctypes.c_void_p()
        _check(_lib.ethrex_mi355_keccak_plan_create(
            ctypes.c_size_t(max_bytes), ctypes.c_size_t(max_n),
            ctypes.byref(self._p)), "keccak_plan_create")

    def upload(self, msgs: bytes, offsets):
        self.n = len(offsets) - 1
        offs = (ctypes.c_uint64 * len(offsets))(*offsets)
        _check(_lib.ethrex_mi355_keccak_upload(
            self._p, _buf(msgs) if msgs else None, offs,
            ctypes.c_size_t(self.n)), "keccak_upload")

    def run(self):
        _check(_lib.ethrex_mi355_keccak_run(self._p), "keccak_run")

    def download(self) -> bytes:
        out = (ctypes.c_uint8 * (32 * self.n))()
        _check(_lib.ethrex_mi355_keccak_download(self._p, out),
               "keccak_download")
        return bytes(out)

    def last_ms(self) -> float:
        ms = ctypes.c_double(0)
        _check(_lib.ethrex_mi355_keccak_last_ms(self._p, ctypes.byref(ms)),
               "keccak_last_ms")
        return ms.value

    def device_digests(self):
        """(device pointer, n) of the last run's 32-byte digests; valid
        until the next upload/destroy (the wrap-binding handoff)."""
        ptr = ctypes.c_void_p()
        nn = ctypes.c_size_t(0)
        _check(_lib.ethrex_mi355_keccak_device_digests(
            self._p, ctypes.byref(ptr), ctypes.byref(nn)),
            "keccak_device_digests")
        return ptr, nn.value

    def destroy(self):
        if self._p:
            _lib.ethrex_mi355_keccak_plan_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class MptBuilder:
    """Native MPT structure builder (host C) with caller-driven per-level
    hashing — §8f row 4 witness-generation speedup.  Fixed 32-byte sorted
    distinct keys (hashed-key state/storage trie shape); see
    include/ethrex_mi355.h and ethrex_amd/trie.py (trie_root_native)."""

    def __init__(self, keys32: bytes, vals: bytes, val_offs):
        self.n = len(val_offs) - 1
        self._p = ctypes.c_void_p()
        offs = (ctypes.c_uint64 * len(val_offs))(*val_offs)
        _check(_lib.ethrex_mi355_mpt_create(
            _buf(keys32), _buf(vals) if vals else (ctypes.c_uint8 * 1)(),
            offs, ctypes.c_size_t(self.n), ctypes.byref(self._p)),
            "mpt_create")
        # reusable level-encode buffers (branch worst case ~580 B/node)
        self._cap = 600 * (2 * self.n + 4) + 4096
        self._buf = (ctypes.c_uint8 * self._cap)()
        self._offs = (ctypes.c_uint64 * (2 * self.n + 4))()

    def max_depth(self) -> int:
        d = ctypes.c_int(0)
        _check(_lib.ethrex_mi355_mpt_max_depth(self._p, ctypes.byref(d)),
               "mpt_max_depth")
        return d.value

    def level_encode(self, depth: int):
        """-> (msg bytes, offsets list) for this level's to-hash nodes"""
        k = ctypes.c_size_t(0)
        _check(_lib.ethrex_mi355_mpt_level_encode(
            self._p, ctypes.c_int(depth), self._buf, self._offs,
            ctypes.c_size_t(self._cap), ctypes.c_size_t(2 * self.n + 3),
            ctypes.byref(k)), "mpt_level_encode")
        nh = k.value
        offs = [self._offs[i] for i in range(nh + 1)]
        return bytes(self._buf[:offs[-1]]), offs

    def level_set_hashes(self, depth: int, hashes: bytes):
        _check(_lib.ethrex_mi355_mpt_level_set_hashes(
            self._p, ctypes.c_int(depth),
            _buf(hashes) if hashes else (ctypes.c_uint8 * 1)(),
            ctypes.c_size_t(len(hashes) // 32)), "mpt_level_set_hashes")

    def root(self) -> bytes:
        out = (ctypes.c_uint8 * 32)()
        _check(_lib.ethrex_mi355_mpt_root(self._p, out), "mpt_root")
        return bytes(out)

    def destroy(self):
        if self._p:
            _lib.ethrex_mi355_mpt_destroy(self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
