"""aurora_amd: an MI355X-native forward / rollout engine for the Aurora model family.

Public surface = the reference's (aurora/__init__.py:3-29).  The cyclone tracker (aurora/tracker.py) follows a roll-out
without moving the predictions off the device: only its search windows travel (aurora_amd/tracker.py).  `scores` verifies a
prediction against truth on the device (aurora_amd/scores.py) and `ensemble_scores` an ensemble of them (CRPS, spread, rank
histogram: aurora_amd/ensemble.py) while `ensemble_quantiles` gives its per-point quantile maps -- median, 10 % / 90 %,
interquartile range -- and the map of the truth's rank among the members (aurora_amd/quantiles.py), and `spectra` gives the zonal power spectra of a prediction, of the truth and of the error
(aurora_amd/spectra.py), and `event_scores` the contingency tables and the fractions skill score of threshold exceedances
(aurora_amd/events.py), and `probability_scores` the Brier score, reliability diagram and ROC of an ensemble's event
probabilities (aurora_amd/probability.py), and `FieldStats` accumulates per-point statistics over the steps of a roll-out or
the members of an ensemble as maps (aurora_amd/fieldstats.py), and `diagnostics` forms the derived fields all of them can
then take -- vorticity, divergence, wind speed, integrated vapour transport -- as a `Batch` (aurora_amd/diagnostics.py), and
`conditional_scores` gives the error by bin of the truth and over its tails, against climatology maps such as those of
`FieldStats` (aurora_amd/conditional.py), and `region_scores` gives the scores of `scores` by region -- latitude bands,
longitude boxes and masks, as scorecards report them (aurora_amd/regions.py), and `conservative_regrid` brings a batch to the
grid of its truth by area-weighted remapping, which `Batch.regrid`'s bilinear sampling is not made for
(aurora_amd/conservative.py), and `objects` labels the connected regions of threshold exceedances -- storms, atmospheric rivers,
heat domes -- with their sizes, centres and peaks (aurora_amd/objects.py), and `field_quantiles` gives the spatial quantiles of
every plane by area or by count, the percentile thresholds those event modules are fed (aurora_amd/field_quantiles.py), and
`object_matches` pairs the objects of two fields -- forecast and truth, or step t and step t + 1 -- by their overlap: intersection
over union, best partner, object POD / FAR / CSI, centroid displacement (aurora_amd/object_matches.py), and `nearest_event` gives
for every grid point the great-circle distance to the nearest event and which point that is, from which `object_separations`
takes what objects that do not touch need: minimum boundary separation, Hausdorff distance, "nearest observed object within
300 km" (aurora_amd/distances.py), and `smooth` takes the mean of a field over a great-circle disc of R kilometres, the step
before thresholding in object-based verification (aurora_amd/smooth.py), and `extrema` finds where a field has its lows and
highs -- the points that are the minimum or maximum of all points within R kilometres -- with the minimum / maximum filter itself
(aurora_amd/extrema.py), and `closed_contours` keeps those of them around which the field rises (falls) by at least delta on every
path to the rim of a disc, the closed-contour criterion of storm counts (aurora_amd/contours.py), and `link_extrema` links the
candidates of two steps by an all-pairs nearest search on the sphere, from which `tracks` numbers the storm tracks of a roll-out
(aurora_amd/links.py), and `sphere_spectra` gives the power spectra by total wavenumber -- the spherical-harmonic analysis of
every plane -- and the kinetic-energy spectrum from vorticity and divergence (aurora_amd/sphere_spectra.py), and
`sphere_analysis`, `sphere_synthesis` and `sphere_filter` give the coefficients of that analysis, the field of a set of
coefficients, and a field truncated or weighted by total wavenumber as a `Batch` on its own grid, which every scorer takes
unchanged (aurora_amd/sphere_transform.py); the reference has no counterpart.
"""

from aurora_amd.batch import Batch, Metadata
from aurora_amd.conditional import ConditionalScores, conditional_scores
from aurora_amd.conservative import conservative_regrid
from aurora_amd.contours import ClosedContours, closed_contours
from aurora_amd.diagnostics import diagnostics
from aurora_amd.distances import NearestEvent, ObjectSeparations, nearest_event, object_separations
from aurora_amd.ensemble import EnsembleScores, ensemble_scores
from aurora_amd.events import EventScores, event_scores
from aurora_amd.extrema import Extrema, extrema
from aurora_amd.field_quantiles import FieldQuantiles, field_quantiles
from aurora_amd.fieldstats import FieldStats
from aurora_amd.links import Links, Tracks, link_extrema, tracks
from aurora_amd.model.aurora import (
    Aurora,
    Aurora12hPretrained,
    AuroraAirPollution,
    AuroraHighRes,
    AuroraPretrained,
    AuroraSmall,
    AuroraSmallPretrained,
    AuroraWave,
)
from aurora_amd.object_matches import ObjectMatches, object_matches
from aurora_amd.objects import Objects, objects
from aurora_amd.probability import ProbabilityScores, probability_scores
from aurora_amd.quantiles import EnsembleQuantiles, ensemble_quantiles
from aurora_amd.regions import Region, Regions, RegionScores, region_scores
from aurora_amd.rollout import rollout, write_rollout
from aurora_amd.scores import Scores, scores
from aurora_amd.smooth import smooth
from aurora_amd.spectra import Spectra, spectra
from aurora_amd.sphere_spectra import SphereSpectra, sphere_spectra
from aurora_amd.sphere_transform import SphereCoefficients, sphere_analysis, sphere_filter, sphere_synthesis
from aurora_amd.tracker import Tracker

__all__ = [
    "Aurora",
    "AuroraPretrained",
    "AuroraSmallPretrained",
    "AuroraSmall",
    "Aurora12hPretrained",
    "AuroraHighRes",
    "AuroraAirPollution",
    "AuroraWave",
    "Batch",
    "Metadata",
    "rollout",
    "write_rollout",
    "scores",
    "Scores",
    "ensemble_scores",
    "EnsembleScores",
    "ensemble_quantiles",
    "EnsembleQuantiles",
    "spectra",
    "Spectra",
    "sphere_spectra",
    "SphereSpectra",
    "sphere_analysis",
    "sphere_synthesis",
    "sphere_filter",
    "SphereCoefficients",
    "event_scores",
    "EventScores",
    "probability_scores",
    "ProbabilityScores",
    "FieldStats",
    "diagnostics",
    "conditional_scores",
    "ConditionalScores",
    "region_scores",
    "Region",
    "Regions",
    "RegionScores",
    "conservative_regrid",
    "objects",
    "Objects",
    "object_matches",
    "ObjectMatches",
    "nearest_event",
    "NearestEvent",
    "object_separations",
    "ObjectSeparations",
    "field_quantiles",
    "FieldQuantiles",
    "smooth",
    "extrema",
    "Extrema",
    "closed_contours",
    "ClosedContours",
    "link_extrema",
    "Links",
    "tracks",
    "Tracks",
    "Tracker",
]
