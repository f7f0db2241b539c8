"""MI355X-native early-exit document-classification inference path (drop-in for the reference's eval hot path).

The directory name carries a hyphen, so import it with ``importlib.import_module("multi-modal-early-exit_amd")``
(or ``import mmee_amd`` — a two-line alias module at the repo root).
"""
from . import config, synth  # noqa: F401
from .config import (EarlyExitHead, EarlyExitInference, EarlyExitStrategy, ExitConfig, ExitRule, ModelConfig,  # noqa: F401
                     POSSIBLE_EXITS, parse_exits)
from . import capi  # noqa: F401,E402
from .engine import (CapturedForward, EarlyExitEngine, EngineOutput, ResultChunk, ResultStream, load_checkpoint_tensors,  # noqa: F401,E402
                     save_checkpoint, unpack_stream_rows)
from .microbatch import MicroBatchedEngine  # noqa: F401,E402
from .modeling import (DiTEEForImageClassification, EEModelOutput, EESequenceClassifierOutput,  # noqa: F401,E402
                       LayoutLMv3EEForSequenceClassification, load_local_processor)
from .policy import Policy, criterion_scan_device, gate_scan_device, lte_scan_device, patience_scan_device, policy_scan_device, rule_scan_device  # noqa: F401,E402
from .policy import QuotaScan, quota_scan_device  # noqa: F401,E402
from . import harness  # noqa: F401,E402
from . import dist  # noqa: F401,E402
from . import sweep  # noqa: F401,E402
from . import calibration  # noqa: F401,E402
from . import metrics  # noqa: F401,E402
from .metrics import ExitReport, exit_report  # noqa: F401,E402
from . import feed  # noqa: F401,E402
from . import heads  # noqa: F401,E402
from .heads import (GateFit, HeadFit, LteFit, MlpGateFit, MlpHeadFit, balanced_class_weights, collect_distill_features,  # noqa: F401,E402
                    collect_embedding_features, collect_exit_features, collect_gate_features, collect_lte_features, fit_distilled_exit_heads,
                    fit_distilled_mlp_exit_heads, fit_exit_heads, fit_gate_heads, fit_lte_classifier, fit_mlp_exit_heads,
                    fit_mlp_gate_heads, gate_targets, lte_targets, reach_weights)
from .heads import EnsembleFit, fit_exit_ensemble  # noqa: F401,E402
from . import cascade  # noqa: F401,E402
from .cascade import CascadeEngine, CascadeOutput  # noqa: F401,E402
from . import audit  # noqa: F401,E402
from .audit import AuditSample, ConsistencyReport  # noqa: F401,E402
from . import risk  # noqa: F401,E402
from .risk import RiskResult, RollingResult, risk_control, rolling_control  # noqa: F401,E402
from .engine import ControllerLog  # noqa: F401,E402
from . import deadline  # noqa: F401,E402
from .engine import DeadlineLog  # noqa: F401,E402
from .deadline import eta_from_logs, eta_to_next_exit  # noqa: F401,E402
from .engine import VisionFirstOutput, VisionPhase  # noqa: F401,E402
