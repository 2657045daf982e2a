"""Prometheus metrics.

The reference registers no custom metrics; BASELINE.json's
north star requires an attach→CDI-ready latency histogram plus reconcile
counters.  Buckets are sized for a composable fabric whose attach path is
dominated by fabric-manager RTT + PCIe rescan + amdgpu bind: sub-second with a
mock fabric, tens of seconds worst-case on real hardware.
"""

from __future__ import annotations

from prometheus_client import Counter, Gauge, Histogram, REGISTRY

_BUCKETS = (
    0.001, 0.0025, 0.005, 0.01, 0.025, 0.05, 0.1, 0.25, 0.5,
    1.0, 2.5, 5.0, 10.0, 30.0, 60.0, 120.0, 300.0,
)


class Metrics:
    """Per-manager metric set (label ``controller`` distinguishes loops).

    prometheus_client registries are process-global; multiple Manager
    instances in one process (tests, bench ranks) share collectors via the
    class-level cache instead of re-registering.
    """

    _singleton = None

    def __new__(cls):
        if cls._singleton is None:
            cls._singleton = super().__new__(cls)
            cls._singleton._init_collectors()
        return cls._singleton

    def _init_collectors(self) -> None:
        self.attach_to_ready_seconds = Histogram(
            "cro_attach_to_ready_seconds",
            "Latency from ComposableResource entering Attaching to Online "
            "status write (CDI spec emitted and device visible)",
            buckets=_BUCKETS,
        )
        self.detach_seconds = Histogram(
            "cro_detach_seconds",
            "Latency from Detaching entry to device removal completion",
            buckets=_BUCKETS,
        )
        self.attach_phase_seconds = Histogram(
            "cro_attach_phase_seconds",
            "Per-phase attach timing (driver gate, fabric RTT, node refresh, "
            "CDI write, health probe) — the reference has no per-phase "
            "tracing (SURVEY.md §5.1)",
            ["phase"],
            buckets=_BUCKETS,
        )
        self.reconcile_total = Counter(
            "cro_reconcile_total",
            "Reconcile invocations by controller and outcome",
            ["controller", "result"],
        )
        self.fabric_request_seconds = Histogram(
            "cro_fabric_request_seconds",
            "Fabric-manager API round-trip time by operation",
            ["provider", "operation"],
            buckets=_BUCKETS,
        )
        self.devices_online = Gauge(
            "cro_devices_online", "ComposableResources currently Online"
        )
        self.probe_integrity_failures_total = Counter(
            "cro_probe_integrity_failures_total",
            "Attaches refused by the deep probe's data-integrity stage, by "
            "the stage that failed (vram, h2d_dma, d2h_dma, h2d_kernel, "
            "d2h_kernel)",
            ["stage"],
        )
        self.probe_compute_failures_total = Counter(
            "cro_probe_compute_failures_total",
            "Attaches refused by the probe's compute-coverage stage, by the "
            "check that failed (mfma_f32, mfma_i8, mfma_bf16, lds; coverage "
            "for the optional CU-coverage floor)",
            ["test"],
        )
        self.probe_formats_failures_total = Counter(
            "cro_probe_formats_failures_total",
            "Attaches refused by the probe's matrix-format stage, by the check "
            "that failed (mfma_f16, mfma_fp8, mfma_bf8, mx_fp8, mx_fp6, mx_fp4, "
            "mfma_f64; coverage for the optional CU-coverage floor)",
            ["test"],
        )
        self.probe_coherence_failures_total = Counter(
            "cro_probe_coherence_failures_total",
            "Attaches refused by the probe's coherence stage, by the check that "
            "failed (add_u32, add_u64, add_f32, add_f64, pk_add_f16, pk_add_bf16, "
            "minmax, bitwise, ticket, cas, lds_rmw, visibility; coverage for the "
            "optional CU-coverage floor)",
            ["test"],
        )
        self.probe_movement_failures_total = Counter(
            "cro_probe_movement_failures_total",
            "Attaches refused by the probe's data-movement stage, by the check "
            "that failed (dpp, swizzle, bpermute, permlane_swap, readlane, "
            "lds_tr16, lds_tr8, lds_tr4, lds_tr6, lds_dma; coverage for the "
            "optional CU-coverage floor)",
            ["test"],
        )
        self.probe_alu_failures_total = Counter(
            "cro_probe_alu_failures_total",
            "Attaches refused by the probe's ALU stage, by the check that failed "
            "(int_arith, bit_ops, pk_int, dot, f32, f16, f64, convert, "
            "scale_convert, compare_select, salu, transcendental; coverage for "
            "the optional CU-coverage floor)",
            ["test"],
        )
        self.scrub_failures_total = Counter(
            "cro_scrub_failures_total",
            "Scrubs before drain that did not pass, by reason (residue: words "
            "still differ after the fill; fraction: less of the VRAM covered "
            "than the floor asks; lds_residue: LDS words still differ after "
            "the fill or at the recheck; lds_coverage: fewer CUs reached than "
            "the floor asks; reg_residue: vector register words still differ "
            "after the fill or at the recheck; reg_coverage: fewer SIMDs "
            "reached than the floor asks; error: the scrub could not run)",
            ["reason"],
        )
        self.scrub_seconds = Histogram(
            "cro_scrub_seconds",
            "Duration of the scrub before drain, allocation included",
            buckets=_BUCKETS,
        )
        self.scrub_bytes_total = Counter(
            "cro_scrub_bytes_total", "Bytes of VRAM overwritten by scrubs before drain"
        )

    # test helper: drop collectors so a fresh interpreter state can be faked
    @classmethod
    def _reset_for_tests(cls) -> None:
        if cls._singleton is not None:
            for collector in (
                cls._singleton.attach_to_ready_seconds,
                cls._singleton.detach_seconds,
                cls._singleton.attach_phase_seconds,
                cls._singleton.reconcile_total,
                cls._singleton.fabric_request_seconds,
                cls._singleton.devices_online,
                cls._singleton.probe_integrity_failures_total,
                cls._singleton.probe_compute_failures_total,
                cls._singleton.probe_formats_failures_total,
                cls._singleton.probe_coherence_failures_total,
                cls._singleton.probe_movement_failures_total,
                cls._singleton.probe_alu_failures_total,
                cls._singleton.scrub_failures_total,
                cls._singleton.scrub_seconds,
                cls._singleton.scrub_bytes_total,
            ):
                try:
                    REGISTRY.unregister(collector)
                except KeyError:
                    pass
            cls._singleton = None
